"""The symbolic phase hands the device the same bytes as before it was cut into stages.

tests/golden/program_digest_parent.json holds, per case, a SHA-1 of everything spicey_build_program gives the rest of the
library (tests/emul/emul.cpp, spicey_emul_program_dump: blob, offsets, orderings, header scalars, return code and error
text, and the resident layouts of the two transient geometries) plus a few counts of the program.  It was recorded by
tools/record_program_digest.py with spicey_amd/csrc/symbolic.cpp at the content of the commit BEFORE the staged builder,
never from the code under test.  The cases walk every path of the builder: both entry numberings, the tridiagonal top on
and off, the hybrid layout, dense fronts with bins (automatic cut with 1 and 64 instances, fixed cuts, the experiment
switches of the front stage), floating sources, source loops, structurally singular matrices, a shorted source, a refused
descriptor.

Return codes: the descriptor check is the only reachable refusal (the `bad_desc` case).  The builder's own early returns
(`ordering lost vertices`, `stamp outside the symbolic pattern`, `hybrid layout met an index on the wrong side`) are
internal consistency checks that no descriptor which passes spicey_check_desc can trip.
"""
from __future__ import annotations

import hashlib
import json
import os

import pytest

from spicey_amd import abi, synth
from spicey_amd.netlist import parseNetlist

from conftest import PROBE_GOLDENS, QUIRK_GOLDENS, SINGULAR_GOLDENS, SMALL_GOLDENS, golden_netlist, load_golden
from emul.pyemul import program_dump

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "program_digest_parent.json")
# every variable the symbolic phase reads: unset unless a case sets it
ENV_KNOBS = ("SPICEY_FRONT_CUT", "SPICEY_FRONT_EXACT", "SPICEY_STAGED_MERGE_MP", "SPICEY_FRONT_CHILD_ORDER_ID", "SPICEY_BINS",
             "SPICEY_DUMP_SECTIONS", "SPICEY_NO_KMERGE")
SHORTED_SOURCE = "* a source across one node\nV1 a a 1\nR1 a 0 1\n.tran 1e-6 1e-5\n.end\n"
CHAINS = [("diode_chain", n) for n in (20, 100, 333, 1000, 2600)] + [("rc_ladder", n) for n in (20, 1000)]
MESHES = (6, 12, 20, 34)
FRONT_MESHES = (12, 20, 34)  # the three largest: fixed and automatic cuts
STAGED_MESH = 74             # smallest mesh (even sizes from 70) with a front beyond LDS residency (max_front_mp = 176 > 128)
# 300 leaves on one hub: the hub's diagonal collects 300 products in one level, more than the 8-bit count of a 16-bit record
# holds, so the builder retreats to the 32-bit lists although the workspace is small (has16 == 0 without fronts)
STAR = "* star\nV1 h 0 1\n" + "".join(f"R{i} h n{i} 1k\nC{i} n{i} 0 1n\n" for i in range(300)) + ".tran 1e-6 1e-5\n.end\n"


def circuits():
    """(name, netlist text, kind)."""
    for gen, n in CHAINS:
        yield f"{gen}({n})", getattr(synth, gen)(n), "chain"
    for r in MESHES:
        yield f"rcd_mesh({r})", synth.rcd_mesh(r), "mesh"
    for name in SMALL_GOLDENS + SINGULAR_GOLDENS + QUIRK_GOLDENS + PROBE_GOLDENS:
        yield f"golden:{name}", golden_netlist(load_golden(name)), "golden"
    yield "shorted_source", SHORTED_SOURCE, "inline"
    yield "star(300)", STAR, "inline"


def cases():
    """(key, circuit name, n_inst, (bank_aware, front_cut, pcr_top, hybrid), environment, bad descriptor?)."""
    out = []
    for name, _, kind in circuits():
        for bank in (0, 1):
            for top in (0, 1):
                out.append((f"{name} bank={bank} top={top}", name, 1, (bank, 0, top, 0), {}, False))
        if kind == "chain":
            for top in (0, 1):
                out.append((f"{name} hybrid top={top}", name, 1, (1, 0, top, 1), {}, False))
    for r in FRONT_MESHES:
        for cut in (-1, 6, 10):
            for n_inst in (1, 64):
                out.append((f"rcd_mesh({r}) cut={cut} inst={n_inst}", f"rcd_mesh({r})", n_inst, (1, cut, 1, 0), {}, False))
    for var, val in (("SPICEY_FRONT_EXACT", "1"), ("SPICEY_BINS", "0"), ("SPICEY_STAGED_MERGE_MP", "0"), ("SPICEY_FRONT_CHILD_ORDER_ID", "1")):
        out.append((f"rcd_mesh(34) cut=-1 {var}={val}", "rcd_mesh(34)", 1, (1, -1, 1, 0), {var: val}, False))
    out.append((f"rcd_mesh({STAGED_MESH}) cut=-1 inst=1", f"rcd_mesh({STAGED_MESH})", 1, (1, -1, 1, 0), {}, False))
    out.append((f"rcd_mesh({STAGED_MESH}) cut=-1 SPICEY_STAGED_MERGE_MP=0", f"rcd_mesh({STAGED_MESH})", 1, (1, -1, 1, 0), {"SPICEY_STAGED_MERGE_MP": "0"}, False))
    out.append(("bad_desc", "diode_chain(20)", 1, (1, 0, 1, 0), {}, True))
    return out


_FLATS: dict = {}


def flat_of(name: str, n_inst: int):
    if not _FLATS:
        for nm, text, _ in circuits():
            _FLATS[(nm, 1)] = abi.flatten(parseNetlist(text), probe_filter=True)
        _FLATS[(f"rcd_mesh({STAGED_MESH})", 1)] = abi.flatten(parseNetlist(synth.rcd_mesh(STAGED_MESH)), probe_filter=True)
    if (name, n_inst) not in _FLATS:
        _FLATS[(name, n_inst)] = _FLATS[(name, 1)].replicate(n_inst)
    return _FLATS[(name, n_inst)]


def record(case) -> dict:
    """The fixture's entry of one case, from the symbolic phase as built now (the caller has set the environment)."""
    _, name, n_inst, args, _, bad = case
    flat = flat_of(name, n_inst)
    desc = flat.desc()
    if bad:
        desc.abi_version = 0
    data, scalars = program_dump(flat, *args, desc=desc)
    return {"sha1": hashlib.sha1(data).hexdigest(), "bytes": len(data), **scalars}


@pytest.fixture(scope="module")
def parent():
    with open(GOLDEN) as f:
        return json.load(f)


def test_the_fixture_holds_exactly_the_cases(parent):
    assert sorted(parent) == sorted(c[0] for c in cases())


@pytest.mark.parametrize("case", cases(), ids=lambda c: c[0])
def test_program_is_byte_identical_to_the_parent(case, parent, monkeypatch):
    for var in ENV_KNOBS:
        monkeypatch.delenv(var, raising=False)
    for var, val in case[4].items():
        monkeypatch.setenv(var, val)
    got = record(case)
    want = parent[case[0]]
    assert sorted(got) == sorted(want)
    assert got == want


def test_the_scan_reaches_every_path_of_the_builder(parent):
    recs = list(parent.values())
    assert any(r["nFronts"] > 0 for r in recs)
    assert any(r["nBins"] > 0 for r in recs)
    assert any(r["hybrid"] == 1 for r in recs)
    assert any(r["pcr_n"] > 0 for r in recs)
    assert any(r["fus_pairs"] > 0 for r in recs)
    assert any(r["ovf16"] > 0 for r in recs)
    assert any(r["rc"] == 0 and r["has16"] == 0 and r["nFronts"] == 0 for r in recs)  # (fronts switch the 16-bit records off too)
    assert any(r["structurally_singular"] for r in recs)
    assert any(r["rc"] != 0 for r in recs)
    assert any(r["max_front_mp"] > 128 for r in recs)
    assert any(r["numbering"] == 2 for r in recs)  # slot-major kept
    assert any(r["numbering"] == 1 for r in recs)  # CSR order kept
    assert parent["diode_chain(1000) bank=1 top=1"]["numbering"] == 2
    assert parent["rcd_mesh(34) cut=10 inst=1"]["nFronts"] > 0 and parent["rcd_mesh(20) cut=10 inst=1"]["nFronts"] > 0
