"""simulateTRANBatch on the CPU: its grouping, its re-keying and state write-back, and its handling of singular instances,
checked through the oracle run instance by instance against a loop of simulateTRAN on the same oracle."""
import re

import numpy as np
import pytest

from batch_variants import PerInstanceOracle, variant
from conftest import SINGULAR_GOLDENS, SMALL_GOLDENS, bits_equal, golden_netlist, load_golden
from spicey_amd import abi
from spicey_amd.batch import batch_launches, simulateTRANBatch
from spicey_amd.netlist import parseNetlist
from spicey_amd.simulate import SingularMatrixError, simulateTRAN

NO_TRAN = "* no transient\nV1 a 0 DC 1\nR1 a 0 1k\n.end\n"
DUP_NAMES = "* two elements named R1\nV1 a 0 DC 2\nR1 a b 1k\nR1 b 0 2k\nC1 b 0 1u\n.tran 1u 20u\n.end\n"


def _texts():
    out = []
    for name in SMALL_GOLDENS:
        text = golden_netlist(load_golden(name))
        out += [text, variant(text, 1), variant(text, 2, values=False)]
    out += [variant(golden_netlist(load_golden("vswitch_pwl")), k, values=False, amplitude=False, pwl_times=True) for k in (1, 2)]
    out += [NO_TRAN, DUP_NAMES, variant(DUP_NAMES, 3)]
    # near_sing_b's topology with a resistor that grounds node x well: solvable, launched with the singular original
    nsb = golden_netlist(load_golden("near_sing_b"))
    out += [nsb.replace("1e16", "1k"), nsb.replace("1e16", "3.3k")]
    # singular circuits mixed in, next to copies of themselves and of good circuits
    for name in SINGULAR_GOLDENS:
        out.insert(3 * SINGULAR_GOLDENS.index(name) + 1, golden_netlist(load_golden(name)))
    return out


def _same_result(a, b, where):
    assert list(a) == list(b), where
    assert a["times"] == b["times"], where
    for part in ("nodeVoltages", "elementCurrents"):
        assert list(a[part]) == list(b[part]), where
        for k in a[part]:
            assert bits_equal(a[part][k], b[part][k]).all(), (where, part, k)
    assert np.array_equal(a["iterations"], b["iterations"]) and a["skipRisk"] == b["skipRisk"], where


def _state(ckt):
    return ([c.vPrev for c in ckt.C], [l.iPrev for l in ckt.L], [d.vdPrev for d in ckt.D], [s.isOn for s in ckt.S])


def test_batch_equals_a_loop_of_simulateTRAN_bit_for_bit():
    texts = _texts()
    batch = [parseNetlist(t) for t in texts]
    solo = [parseNetlist(t) for t in texts]
    be = PerInstanceOracle()
    for rnd in range(2):  # the second call continues from the state the first one wrote
        before = [_state(c) for c in batch]
        got = simulateTRANBatch(batch, backend=be)
        assert len(got) == len(texts)
        for i, (g, c) in enumerate(zip(got, solo)):
            try:
                ref = simulateTRAN(c, backend=PerInstanceOracle())
            except SingularMatrixError:
                assert isinstance(g, SingularMatrixError), (rnd, i)
                assert _state(batch[i]) == before[i], (rnd, i)  # untouched
                continue
            if ref is None:
                assert g is None, (rnd, i)
                continue
            _same_result(g, ref, (rnd, i))
            assert _state(batch[i]) == _state(c), (rnd, i)
    # fewer launches than circuits: variants shared one, and none ran a follow-up (the oracle stops nobody)
    assert len(be.launches) < len([t for t in texts if ".tran" in t])
    assert any(n > 1 and per for n, per in be.launches)


def test_singular_instance_keeps_its_state_and_neighbours_match():
    text = golden_netlist(load_golden("near_sing_b"))
    good = [variant(golden_netlist(load_golden("dchain20")), k) for k in range(3)]
    batch = [parseNetlist(t) for t in good[:1] + [text] + good[1:]]
    got = simulateTRANBatch(batch, backend=PerInstanceOracle())
    assert isinstance(got[1], SingularMatrixError) and str(got[1]) == "Singular matrix (real)"
    for g, t in zip([got[0], got[2], got[3]], good):
        _same_result(g, simulateTRAN(parseNetlist(t), backend=PerInstanceOracle()), t[:20])


class _Mates(PerInstanceOracle):
    """Like the GPU with two instances per workgroup: a singular instance stops its workgroup mate unfinished (-1)."""

    def run(self, flat, steps, dt, src, want_currents=True, want_iters=True):
        res = super().run(flat, steps, dt, src, want_currents, want_iters)
        for j in np.nonzero(res["inst_status"] == abi.ERR_SINGULAR)[0]:
            mate = j ^ 1
            if mate < flat.n_inst and res["inst_status"][mate] == 0:
                res["inst_status"][mate] = -1
                res["out_v"][mate] = np.nan  # (what it left is not a result)
        return res


def test_instances_stopped_by_a_workgroup_mate_run_again():
    bad = golden_netlist(load_golden("near_sing_b"))  # singular; the same topology with 1k or 2k from x to ground is not
    texts = [bad.replace("1e16", "1k"), bad.replace("1e16", "2k")]
    be = _Mates()
    got = simulateTRANBatch([parseNetlist(texts[0]), parseNetlist(bad), parseNetlist(texts[1])], backend=be)
    assert isinstance(got[1], SingularMatrixError)
    for i, t in ((0, texts[0]), (2, texts[1])):
        _same_result(got[i], simulateTRAN(parseNetlist(t), backend=PerInstanceOracle()), i)
    assert [n for n, _ in be.launches] == [3, 1]  # instance 0 was stopped by its mate and ran again alone


class _DiagnosticsOnlyOnSuccess(PerInstanceOracle):
    """A backend that returns the finished instances' results after a singular run, but their skip counts only when the
    whole run succeeded."""

    def run(self, flat, steps, dt, src, want_currents=True, want_iters=True):
        res = super().run(flat, steps, dt, src, want_currents, want_iters)
        if res["status"] != abi.OK:
            del res["skip_risk"]
        return res


def skip_island(val):
    """skip_quirk (the reference drops multipliers: nonzero skip counts) with an island x grounded through `val`, which
    is singular at 1e16 ohm (near_sing_b) and solvable otherwise: one topology."""
    return golden_netlist(load_golden("skip_quirk")).replace(".tran", f"R9 x 0 {val}\n.tran")


def test_skip_counts_of_neighbours_of_a_singular_instance():
    texts = [skip_island("1k"), skip_island("1e16"), variant(skip_island("2.2k"), 1, values=False)]
    solo = [simulateTRAN(parseNetlist(t), backend=PerInstanceOracle()) if i != 1 else None for i, t in enumerate(texts)]
    assert solo[0]["skipRisk"] > 0 and solo[2]["skipRisk"] > 0
    for be in (PerInstanceOracle(), _DiagnosticsOnlyOnSuccess()):
        got = simulateTRANBatch([parseNetlist(t) for t in texts], backend=be)
        assert isinstance(got[1], SingularMatrixError)
        for i in (0, 2):
            _same_result(got[i], solo[i], i)
        # without diagnostics after the failure the finished instances are not reported with a made-up count: they run again
        assert [n for n, _ in be.launches] == ([3] if type(be) is PerInstanceOracle else [3, 2])


def test_a_table_that_differs_only_in_the_sign_of_a_zero_is_its_own():
    base = "* a source at zero\nV1 a 0 DC 0\nR1 a b 1k\nC1 b 0 1n\n.tran 1e-6 4e-6\n.end\n"
    ckts = [parseNetlist(base), parseNetlist(base)]
    ckts[0].V[0].waveform = lambda t: 0.0
    ckts[1].V[0].waveform = lambda t: -0.0  # (equal to 0.0 as a number, not as the reference's value)
    be = PerInstanceOracle()
    simulateTRANBatch(ckts, backend=be)
    assert be.launches == [(2, True)]


def test_grouping():
    rc = golden_netlist(load_golden("readme_rc"))
    lad = golden_netlist(load_golden("ladder20"))
    probe2 = golden_netlist(load_golden("two_probes"))
    other_dt = re.sub(r"(?m)^\.tran .*$", ".tran 2e-9 2e-6", rc)
    c = [parseNetlist(t) for t in (rc, lad, variant(rc, 1), NO_TRAN, variant(lad, 2), other_dt)]
    launches = batch_launches(c)
    assert launches[0] == [0, 2] and launches[1] == [1, 4]
    assert all(3 not in l for l in launches)
    # another dt / stop time: a launch of its own
    assert len(launches) == 3 and launches[2] == [5]
    # split into consecutive launches
    many = [parseNetlist(variant(lad, k % 4)) for k in range(7)]
    assert batch_launches(many, max_instances=3) == [[0, 1, 2], [3, 4, 5], [6]]
    # the recorded nodes are part of the key: two_probes without its .PRINT records every node
    noprint = probe2.replace(".PRINT", "*.PRINT")
    assert batch_launches([parseNetlist(probe2), parseNetlist(noprint), parseNetlist(variant(probe2, 1))]) == [[0, 2], [1]]
    # another element order is another topology
    a = "V1 a 0 DC 1\nR1 a b 1k\nR2 b 0 1k\n.tran 1u 5u\n"
    b = "V1 a 0 DC 1\nR2 b 0 1k\nR1 a b 1k\n.tran 1u 5u\n"
    assert batch_launches([parseNetlist(a), parseNetlist(b), parseNetlist(a.replace("1k", "2k"))]) == [[0, 2], [1]]
    with pytest.raises(ValueError):
        batch_launches(many, max_instances=0)


def test_shared_table_when_every_table_is_equal():
    lad = golden_netlist(load_golden("ladder20"))
    be = PerInstanceOracle()
    simulateTRANBatch([parseNetlist(variant(lad, k, amplitude=False)) for k in range(3)], backend=be)
    simulateTRANBatch([parseNetlist(variant(lad, k)) for k in range(3)], backend=be)
    assert be.launches == [(3, False), (3, True)]


def test_same_circuit_twice_is_refused_and_no_tran_gives_none():
    c = parseNetlist(golden_netlist(load_golden("readme_rc")))
    with pytest.raises(ValueError):
        simulateTRANBatch([c, c], backend=PerInstanceOracle())
    assert simulateTRANBatch([parseNetlist(NO_TRAN)], backend=PerInstanceOracle()) == [None]
    with pytest.raises(ValueError):
        simulateTRANBatch([c], backend=PerInstanceOracle(), exact_order=True)


def test_source_tables_stack_the_circuits_tables():
    texts = [variant(golden_netlist(load_golden("two_probes")), k) for k in range(3)]
    ckts = [parseNetlist(t) for t in texts]
    dt, steps = abi.computeEffectiveTimeStep(ckts[0].analyses["tran"]["dt"], ckts[0].analyses["tran"]["tstop"])
    tabs = abi.source_tables(ckts, dt, steps)
    assert tabs.shape == (3, steps + 1, 1)
    for c, t in zip(ckts, tabs):
        assert np.array_equal(t, abi.source_table(c, dt, steps))
    assert not np.array_equal(tabs[0], tabs[1])
    with pytest.raises(ValueError):
        abi.source_tables([ckts[0], parseNetlist(DUP_NAMES.replace("V1 a 0 DC 2", "V1 a 0 DC 2\nV2 b 0 DC 1"))], dt, steps)
