"""simulateACBatch on the CPU: the grouping, the stacking of per-instance values and phasors, the re-keying and the
per-slot errors, with the oracle (oracle/pyoracle.py, run instance by instance) behind the batch backend interface."""
import numpy as np
import pytest

from batch_variants import instance, variant
from conftest import golden_netlist, load_golden
from spicey_amd import abi
from spicey_amd import ac as sac
from spicey_amd.ac_batch import simulateACBatch
from spicey_amd.netlist import parseNetlist


class PerInstanceAcOracle:
    """The oracle behind run_ac of a batch backend: every instance on its own with its own phasors, results of the instances
    that are fine also after a failing one, `inst_status` / `first_freq` like AcHandle.run.  It is the reference's own
    algorithm, frequency by frequency, so like the reference-order engine it raises an inductor's divide error itself."""

    exact_order = True

    def __init__(self):
        from oracle.pyoracle import OracleBackend
        self.be = OracleBackend()
        self.launches = []  # instance count of every run_ac

    def run_ac(self, flat, freqs, vph, want_currents=True):
        ni, nf = flat.n_inst, len(freqs)
        self.launches.append(ni)
        vph = np.broadcast_to(np.asarray(vph, np.complex128).reshape(-1, flat.nV), (ni, flat.nV))
        res = {"status": abi.OK, "detail": "", "out_v": np.zeros((ni, nf, flat.n_nodes), np.complex128),
               "out_i": np.zeros((ni, nf, flat.nR + flat.nC + flat.nL + flat.nV), np.complex128) if want_currents else None,
               "inst_status": np.zeros(ni, np.int32)}
        for j in range(ni):
            r = self.be.run_ac(instance(flat, j), freqs, vph[j], want_currents)
            if r["status"] != abi.OK:
                res["inst_status"][j] = r["status"]
                if res["status"] == abi.OK:
                    res["status"], res["detail"] = r["status"], r["detail"]
                continue
            res["out_v"][j] = r["out_v"][0]
            if want_currents:
                res["out_i"][j] = r["out_i"][0]
        return res


def same_result(a, b):
    assert list(a) == list(b) == ["freqs", "nodeVoltages", "elementCurrents"]
    assert a["freqs"] == b["freqs"]
    for part in ("nodeVoltages", "elementCurrents"):
        assert list(a[part]) == list(b[part])
        for k in a[part]:
            x, y = np.asarray(a[part][k], np.complex128), np.asarray(b[part][k], np.complex128)
            assert x.shape == y.shape and x.tobytes() == y.tobytes(), (part, k)


def texts():
    base = {n: golden_netlist(load_golden(n)) for n in ("ac_rlc", "ac_two_src", "ac_readme")}
    return [variant(base[n], k) for k in range(6) for n in ("ac_rlc", "ac_two_src", "ac_readme")]  # interleaved


def test_batch_equals_solo_and_launches_once_per_topology(oracle_backend):
    ts = texts()
    be = PerInstanceAcOracle()
    got = simulateACBatch([parseNetlist(t) for t in ts], backend=be)
    assert be.launches == [6, 6, 6]
    for t, g in zip(ts, got):
        same_result(g, sac.simulateAC(parseNetlist(t), backend=oracle_backend))
    # the variants differ (the batch did not hand everyone instance 0)
    assert got[0]["nodeVoltages"]["out"] != got[3]["nodeVoltages"]["out"]
    be2 = PerInstanceAcOracle()
    got2 = simulateACBatch([parseNetlist(t) for t in ts], backend=be2, max_instances=2)
    assert be2.launches == [2] * 9
    be3 = PerInstanceAcOracle()
    n_rlc = parseNetlist(ts[0])
    per = 41 * (4 + 6) * 16  # ac_rlc: 41 frequencies x (4 nodes + 6 currents) complex
    got3 = simulateACBatch([parseNetlist(t) for t in ts[0::3]], backend=be3, max_result_bytes=4 * per + 1)
    assert be3.launches == [4, 2] and len(n_rlc.R) + len(n_rlc.C) + len(n_rlc.L) + len(n_rlc.V) == 6
    for a, b in zip(got2, got):
        same_result(a, b)
    for a, b in zip(got3, got[0::3]):
        same_result(a, b)


def test_three_launches_with_max_instances_two_per_topology():
    """One topology, six variants, max_instances=2: three launches."""
    base = golden_netlist(load_golden("ac_rlc"))
    be = PerInstanceAcOracle()
    simulateACBatch([parseNetlist(variant(base, k)) for k in range(6)], backend=be, max_instances=2)
    assert be.launches == [2, 2, 2]


def test_errors_and_none_stay_in_their_slots(oracle_backend):
    good = golden_netlist(load_golden("ac_readme"))
    names = ["ac_none", None, "ac_err_r0", "ac_sing_first", None, "ac_cdiv_last", None]
    ts = [golden_netlist(load_golden(n)) if n else variant(good, k) for k, n in enumerate(names)]
    be = PerInstanceAcOracle()
    got = simulateACBatch([parseNetlist(t) for t in ts], backend=be)
    assert got[0] is None
    assert isinstance(got[2], ValueError) and str(got[2]) == load_golden("ac_err_r0")["error"] == "R R1 must be > 0"
    assert isinstance(got[3], sac.SingularComplexMatrixError) and str(got[3]) == load_golden("ac_sing_first")["error"]
    assert isinstance(got[5], ZeroDivisionError) and str(got[5]) == load_golden("ac_cdiv_last")["error"]
    for k in (1, 4, 6):
        same_result(got[k], sac.simulateAC(parseNetlist(ts[k]), backend=oracle_backend))
    assert sorted(be.launches) == [1, 1, 3]  # (the refused circuit and the one without .ac took part in no launch)
    with pytest.raises(ValueError):
        simulateACBatch([], backend=be, max_instances=0)
    with pytest.raises(ValueError):
        simulateACBatch([], backend=be, exact_order=True)
