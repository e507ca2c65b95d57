"""Operand-address builds (tran_v2_run.h: OA) on the CPU: the packed layout (512 threads, 4 slots) of the fresh
ready-argument build whose always-executed LDS operands are named by handles (tran_common.h: SpiceyOperand) and whose
descriptor fields of phase B index from the start of the workspace — against the same build without all that: same bits
in voltages, currents, iteration counts and end state, also from an arena that starts as NaN and with the threads of
every phase in reverse order.  On the host a handle is the index itself, so what these runs exercise is the prologue's
re-encoding and every read and write through W[field] inside an arena of exactly the kernel's LDS size.  The re-encoded
fields are held against their formulas for instances 0 and 2 of three.  Also the launch plan's decision: with
SPICEY_NO_OPERAND_ADDR, at and one beyond the largest index a field holds, for a hybrid shape and for K != 1.

The harness is tests/addr_host (it compiles the emulator's sources unchanged)."""
from __future__ import annotations

import numpy as np
import pytest

from spicey_amd import synth

from addr_host import pyaddr
from batch_variants import instance
from test_packed_resident_gpu import _switched_ladder

STEPS = 64
KNOBS = ("SPICEY_NO_OPERAND_ADDR", "SPICEY_NO_READY_ARGS", "SPICEY_NO_OPERAND_SLOTS", "SPICEY_NO_EARLY_PREFETCH", "SPICEY_NO_PHASE_TABLE", "SPICEY_NO_FRESH_FILL")


def _chain(n, seeds=(3,)):
    flat, dt, steps, src = synth.chain_batch("diode_chain", n, list(seeds), tran=".tran 1e-6 7e-5")
    assert steps >= STEPS
    return flat, dt, src[: STEPS + 1]


def _switched_one():
    flat, dt, src = _switched_ladder()
    return instance(flat, 2), dt, src


CASES = {
    "diode_chain_100": lambda: _chain(100),     # most threads own no item: every field of their descriptors names a slot
    "diode_chain_1000": lambda: _chain(1000),   # the bench circuit
    "switched_ladder": _switched_one,           # B and the solve run twice in a step, with a_reiterate between them
}
_OFF: dict = {}


def _off_run(case):
    """The ready-argument build without operand addresses: computed once per case, never modified."""
    if case not in _OFF:
        flat, dt, src = CASES[case]()
        r = pyaddr.run(flat, STEPS, dt, src, addr=False)
        assert r["status"] == 0 and r["fresh_fill"] == 1
        for a in (r["out_v"], r["out_i"], r["iters"], *r["state"].values()):
            a.setflags(write=False)
        _OFF[case] = (flat, dt, src, r)
    return _OFF[case]


def _same(got, ref, what):
    for k in ("out_v", "out_i", "iters"):
        assert np.array_equal(got[k], ref[k]), (what, k)
    for k, v in ref["state"].items():
        assert np.array_equal(got["state"][k], v), (what, k)


@pytest.mark.parametrize("variant", ["zeroed", "nan_arena", "reversed"])
@pytest.mark.parametrize("case", sorted(CASES))
def test_operand_addresses_give_the_bits_of_the_indexed_reads(case, variant):
    flat, dt, src, ref = _off_run(case)
    got = pyaddr.run(flat, STEPS, dt, src, addr=True, nan_fill=variant != "zeroed", reverse=variant == "reversed")
    assert got["status"] == 0 and got["slots_fit"] == 1 and got["addr_fits"] == 1 and got["pcr_n"] > 0
    assert np.isfinite(got["out_v"]).all() and np.isfinite(got["out_i"]).all()
    _same(got, ref, (case, variant))
    assert int(got["iters"].min()) >= 1
    if case == "switched_ladder":
        assert got["nS"] > 0 and int(got["iters"].max()) > 1
    assert not np.array_equal(got["state"]["C_vprev"], flat.C_vprev)  # (the run did move the state)


def _want(f, mask, base, minus0):
    """The re-encoded field of a raw descriptor field `f` (index + 1 under `mask`, 0: empty): an index from the start of W."""
    return (f & mask) - 1 + base if f else minus0


def test_reencoded_fields_follow_their_formulas():
    """dd: old index + nW + nU; rhs: old index + nW; an empty field and every field of an item that does not exist: the -0.0
    slot; signs and flags where they were.  Z's terminal halves: ground names the +0.0 slot."""
    flat, dt, src = _chain(100, seeds=(3, 4, 5))
    assert flat.n_inst == 3
    on = pyaddr.run(flat, STEPS, dt, src, addr=True)
    off = pyaddr.run(flat, STEPS, dt, src, addr=False)
    assert on["status"] == 0 and off["status"] == 0
    _same(on, off, "three instances")
    assert not np.array_equal(on["out_v"][0], on["out_v"][2])
    nW, nU, nG, plus0 = on["nW"], on["nU"], on["nGdyn"], on["slot_index"]
    minus0 = plus0 + 1
    assert on["max_index"] == minus0 <= 0x3FFF and minus0 == on["arena_doubles"] - 1  # the two slots are the arena's last doubles
    reg = {k: i for i, k in enumerate(pyaddr.REG_FIELDS)}
    raw = on["raw"].astype(np.int64)
    seen = {"dd": 0, "dd_empty": 0, "rhs": 0, "rhs_empty": 0, "sub": 0}
    for g in (0, 2):
        r, ro = on["regs"][g].astype(np.int64), off["regs"][g].astype(np.int64)
        for t in range(512):
            for j in (0, 1):
                w = int(raw[t][j])
                mine = not (w >> 31)
                got = int(r[t][reg[f"dd{j}"]])
                for q, sh in ((0, 0), (1, 15)):
                    f = (w >> sh) & 0x7FFF if mine else 0
                    assert (got >> sh) & 0x3FFF == _want(f, 0x3FFF, nW + nU, minus0), (g, t, j, q)
                    assert (got >> (sh + 14)) & 1 == ((f >> 14) & 1 if f else 0)  # subtract
                    seen["dd" if f else "dd_empty"] += 1
                    # ... and it is the operand-slot build's field moved by nW + nU
                    assert (got >> sh) & 0x3FFF == ((int(ro[t][reg[f"dd{j}"]]) >> sh) & 0x3FFF) + nW + nU
                assert got >> 30 == (w >> 30 if mine else 2)  # reciprocal / not mine to stamp
                d0, d1 = int(raw[t][2 + 2 * j]), int(raw[t][3 + 2 * j])
                row = d1 != 0xFFFFFFFF
                g0, g1 = int(r[t][reg[f"rhs{j}0"]]), int(r[t][reg[f"rhs{j}1"]])
                for q, (f, gq) in enumerate(((d0 & 0xFFFF, g0 & 0xFFFF), (d0 >> 16, g0 >> 16), (d1 & 0xFFFF, g1 & 0xFFFF), (d1 >> 16, g1 >> 16))):
                    f = f if row else 0
                    assert gq & 0x3FFF == _want(f, 0x7FFF, nW, minus0), (g, t, j, q)
                    assert gq >> 15 == ((f >> 15) if f else 0)  # subtract
                    seen["rhs" if f else "rhs_empty"] += 1
                    seen["sub"] += gq >> 15
                assert (g1 >> 30) & 1 == (0 if row else 1)  # not a resident row
                assert (g0 & 0x3FFF3FFF) == (int(ro[t][reg[f"rhs{j}0"]]) & 0x3FFF3FFF) + nW * 0x10001
                # Z's terminals: a half is a node's index in W, or the +0.0 slot for ground and for an item that does not exist
                for k in ("eR", "eC", "eD"):
                    ab = int(r[t][reg[f"{k}{j}"]])
                    for h in (ab & 0xFFFF, ab >> 16):
                        assert h == plus0 or h < nW
                    assert ab == int(ro[t][reg[f"{k}{j}"]])
    assert all(v > 0 for v in seen.values()), seen  # every kind of field occurred
    # every diode and capacitor of the chain goes to ground: the +0.0 slot on one terminal position of each
    r0 = on["regs"][0].astype(np.int64)
    assert int(np.sum((r0[:, reg["eD0"]] >> 16) == plus0)) == 512 and int(np.sum((r0[:, reg["eD0"]] & 0xFFFF) == plus0)) == 512 - 99


def _synthetic_at(max_index):
    """nW of a synthetic header (nU = 2000, nGdyn = 999, no switches, a top of 64 rows) whose -0.0 slot has this index."""
    for nW in range(1, 40000):
        if pyaddr.fits(nW, 2000, 999)["max_index"] == max_index:
            return nW
    raise AssertionError("no such header")


def test_plan_takes_operand_addresses_where_the_conditions_hold(monkeypatch):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    flat, _, _ = _chain(1000)
    flat = flat.replicate(3)
    on = pyaddr.plan(flat, steps=10000, geometry=2)
    assert on["rc"] == 0 and (on["packed"], on["fresh"], on["early"], on["slots"], on["ready"], on["addr"], on["threads"]) == (1, 1, 1, 1, 1, 1, 512)
    assert (on["ready_run"], on["addr_run"], on["info_operand_addr"]) == (1, 1, 1)
    # a run that the ready-argument kernel does not take has no operand-address form either
    beyond = pyaddr.plan(flat, steps=2**32 - 1, geometry=2)
    assert (beyond["addr"], beyond["ready_run"], beyond["addr_run"]) == (1, 0, 0)
    # the knob: the same plan, the ready-argument kernel without operand addresses
    monkeypatch.setenv("SPICEY_NO_OPERAND_ADDR", "1")
    off = pyaddr.plan(flat, steps=10000, geometry=2)
    assert off["rc"] == 0 and (off["packed"], off["fresh"], off["early"], off["slots"], off["ready"], off["addr"]) == (1, 1, 1, 1, 1, 0)
    assert (off["ready_run"], off["addr_run"], off["info_operand_addr"]) == (1, 0, 0) and off["lds_bytes"] == on["lds_bytes"]
    monkeypatch.delenv("SPICEY_NO_OPERAND_ADDR")
    # the form rides on the ready-argument kernel: without that one, none runs
    monkeypatch.setenv("SPICEY_NO_READY_ARGS", "1")
    p = pyaddr.plan(flat, steps=10000, geometry=2)
    assert (p["ready"], p["ready_run"], p["addr_run"]) == (0, 0, 0)
    monkeypatch.delenv("SPICEY_NO_READY_ARGS")
    # another shape: the latency geometry has no such kernel
    lat = pyaddr.plan(flat, steps=10000, geometry=1)
    assert lat["rc"] == 0 and (lat["packed"], lat["addr"], lat["addr_run"], lat["info_operand_addr"]) == (0, 0, 0, 0)


def test_the_largest_index_a_field_holds_is_accepted_and_one_more_is_refused(monkeypatch):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    at = _synthetic_at(0x3FFF)
    a = pyaddr.fits(at, 2000, 999)
    assert a["field_max"] == 0x3FFF and a["max_index"] == 0x3FFF
    assert (a["slots_fit"], a["addr_fits"], a["plan_addr"], a["ready_run"], a["addr_run"]) == (1, 1, 1, 1, 1)
    # (the tail area is 16-byte aligned, so +0.0 has an even index and -0.0 an odd one: the next header's is 0x4001, and
    # no header puts it at 0x4000)
    assert pyaddr.fits(at + 1, 2000, 999)["max_index"] == 0x3FFF
    over = _synthetic_at(0x4001)
    assert over == at + 2
    b = pyaddr.fits(over, 2000, 999)
    assert b["max_index"] == 0x4001
    # ... refused, and the run takes the ready-argument kernel as before (the operand slots themselves still fit their 16 bits)
    assert (b["slots_fit"], b["addr_fits"], b["plan_addr"], b["ready_run"], b["addr_run"]) == (1, 0, 0, 1, 0)
    # the knob refuses the one that fits
    monkeypatch.setenv("SPICEY_NO_OPERAND_ADDR", "1")
    c = pyaddr.fits(at, 2000, 999)
    assert (c["addr_fits"], c["plan_addr"], c["addr_run"], c["ready_run"]) == (1, 0, 0, 1)


def test_a_hybrid_shape_and_more_than_one_instance_per_workgroup_are_refused(monkeypatch):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    sh = pyaddr.shapes()
    ok = pyaddr.fits(5968, 2000, 999)
    assert (ok["shape_addr"], ok["addr_fits"], ok["plan_addr"]) == (1, 1, 1)
    # a hybrid program on the kernel's own shape, and a hybrid shape
    hyb = pyaddr.fits(5968, 2000, 999, hybrid=1)
    assert (hyb["addr_fits"], hyb["plan_addr"], hyb["addr_run"]) == (0, 0, 0)
    hs = pyaddr.fits(5968, 2000, 999, shape=sh["hybrid"])
    assert sh["hybrid"] >= 0 and (hs["shape_addr"], hs["plan_addr"], hs["addr_run"]) == (0, 0, 0)
    # the packed shape of the default program has no such kernel
    ds = pyaddr.fits(5968, 2000, 999, shape=sh["packed_default"])
    assert sh["packed_default"] >= 0 and sh["packed_default"] != sh["packed_fresh"] and (ds["shape_addr"], ds["plan_addr"]) == (0, 0)
    # K != 1: the workspace interleaves instances, a field is no address
    for K in (2, 4):
        k2 = pyaddr.fits(5968, 2000, 999, K=K)
        assert (k2["addr_fits"], k2["plan_addr"], k2["addr_run"]) == (1, 0, 0)
    # and a real circuit planned with two instances per workgroup
    flat, _, _ = _chain(100, seeds=(3, 4))
    p = pyaddr.plan(flat, steps=64, inst_per_wg=2)
    assert p["rc"] == 0 and p["inst_per_wg"] == 2 and (p["addr"], p["addr_run"], p["info_operand_addr"]) == (0, 0, 0)
