"""optimizeTRAN on the GPU (spicey_run_fit through HipBackend): the device loop equals the host loop on the same backend bit for
bit; the returned circuit reproduces the returned scalars; the CPU oracle's simulation of it meets the goals; three starts in one
handle, one of them singular; the handle after the call.

The margin of the oracle check is derived, not tuned.  The device stops at its own cost F = sum_j r_j^2, so each of its residuals
is at most sqrt(F) in magnitude.  The oracle's transient differs from the device's by at most the parity bar 1e-9 |v| + 1e-12 per
sample; final is one sample and avg a mean of samples, so each scalar moves by at most that bar and each residual by at most
w_j (1e-9 |x_j| + 1e-12).  Hence |r_j(oracle)| <= sqrt(F) + w_j (1e-9 |x_j| + 1e-12): the device's own stopping rule plus the
parity bar, as the bound 2 of test_pss_run_gpu.py is 1 + 1.  Iteration counts are printed, and apart from max_iter not asserted."""
import copy
import math

import numpy as np
import pytest

from spicey_amd import abi, fit, optimizeTRAN
from spicey_amd.fit import at_most, target
from spicey_amd.measure import measureTRAN, stats
from spicey_amd.netlist import parseNetlist

pytestmark = pytest.mark.gpu

# a loaded RC low-pass behind a 5 V step from the zero state; R3 hangs a node of its own to ground and touches no goal
RC = "V1 in 0 5\nR1 in out 1000\nC1 out 0 2e-9\nR2 out 0 2000\nR3 x 0 1000\n.tran 4e-7 4e-5\n.end\n"
MEASURES = {"o": stats("v(out)")}
GOALS = {"o.final": target(3.0, scale=0.01), "o.avg": at_most(2.95, scale=0.01)}   # an EQ goal and an AT_MOST goal (exceeded at the start)
VARS = {"R1": (200.0, 5000.0), "R2": (500.0, 8000.0)}
MAX_ITER = 30
_RUN = {}


class _HostLoop:
    """A backend without run_fit: optimizeTRAN drives it through host_run_fit."""

    def __init__(self, be):
        self._be = be

    def __getattr__(self, name):
        if name == "run_fit":
            raise AttributeError(name)
        return getattr(self._be, name)


def _runs():
    if not _RUN:
        from spicey_amd.lib import HipBackend
        _RUN["ckt"] = parseNetlist(RC)
        _RUN["dev"] = optimizeTRAN(_RUN["ckt"], MEASURES, GOALS, VARS, max_iter=MAX_ITER, backend=HipBackend())
        _RUN["host"] = optimizeTRAN(parseNetlist(RC), MEASURES, GOALS, VARS, max_iter=MAX_ITER, backend=_HostLoop(HipBackend()))
    return _RUN["ckt"], _RUN["dev"], _RUN["host"]


def _bits(d):
    return {k: np.float64(v).view(np.int64) for k, v in d.items()}


def test_device_loop_equals_the_host_loop_bit_for_bit():
    """The same design products, the same transient kernels, the same passes and scalars, the same update."""
    _, dev, host = _runs()
    print("device iterations", dev["iterations"], "status", dev["status"], "cost", dev["cost"], "fit_ms", dev["fit_ms"], "kernel_ms", dev["kernel_ms"])
    assert 1 <= dev["iterations"] <= MAX_ITER and dev["iterations"] == host["iterations"] and dev["status"] == host["status"]
    for n, (a, b) in enumerate(zip(dev["history"], host["history"])):
        assert _bits(a) == _bits(b), (n, a, b)
    assert _bits(dev["values"]) == _bits(host["values"]) and _bits(dev["scalars"]) == _bits(host["scalars"]) and _bits({"F": dev["cost"]}) == _bits({"F": host["cost"]})
    assert dev["history"][0]["accepted"] == 1.0 and dev["history"][0]["F"] > dev["cost"]
    assert dev["fit_ms"] > 0.0 and dev["kernel_ms"] > 0.0


def test_returned_circuit_reproduces_the_scalars_and_the_oracle_meets_the_goals():
    from oracle.pyoracle import OracleBackend
    from spicey_amd.lib import HipBackend
    ckt, dev, _ = _runs()
    assert dev["converged"] and dev["status"] == 0
    assert (ckt.R[0].R, ckt.R[1].R) == (1000.0, 2000.0)   # the input is not mutated
    # (measureTRAN writes the end state back into its circuit: each simulation gets a copy of its own)
    got = measureTRAN(copy.deepcopy(dev["circuit"]), MEASURES, backend=HipBackend())["o"]
    assert _bits({"o.final": got["final"], "o.avg": got["avg"]}) == _bits(dev["scalars"])
    ref = measureTRAN(copy.deepcopy(dev["circuit"]), MEASURES, backend=OracleBackend())["o"]
    root_f = math.sqrt(dev["cost"])
    for key, x_dev, x_ref in (("o.final", got["final"], ref["final"]), ("o.avg", got["avg"], ref["avg"])):
        _, kind, lo, hi, w = GOALS[key]
        r = w * (x_ref - lo) if kind == abi.FIT_EQ else w * max(x_ref - hi, 0.0)
        margin = root_f + w * (1e-9 * abs(x_dev) + 1e-12)
        print(f"{key}: device {x_dev!r}, oracle {x_ref!r}, oracle residual {r:.3e}, margin {margin:.3e}")
        assert abs(r) <= margin


def test_three_starts_in_one_handle_one_of_them_singular():
    """Start 2 puts R3, the only element at its node, at 1e16 ohms: every instance of that problem is singular, its first nominal is
    not evaluable (status 2) and it is frozen; the others go on and converge.  One instance per workgroup, so that the failing
    instances stop nobody else."""
    from spicey_amd.lib import HipBackend
    vars3 = dict(VARS, R3=(100.0, 1e17))
    r = optimizeTRAN(parseNetlist(RC), MEASURES, GOALS, vars3, starts=[{}, {"R1": 1500.0, "R2": 2500.0}, {"R3": 1e16}], max_iter=MAX_ITER,
                     backend=HipBackend(inst_per_wg=1))
    s = r["starts"]
    print("iterations", [q["iterations"] for q in s], "status", [q["status"] for q in s], "cost", [q["cost"] for q in s])
    assert [q["status"] for q in s] == [0, 0, abi.FIT_NOT_EVALUABLE] and s[2]["iterations"] == 1 and s[2]["cost"] == math.inf
    assert s[2]["values"] == {"R1": 1000.0, "R2": 2000.0, "R3": 1e16} and r["best_start"] in (0, 1) and r["converged"]
    for q in s[:2]:
        assert q["values"]["R3"] == 1000.0 and abs(q["scalars"]["o.final"] - 3.0) <= 0.01 * math.sqrt(q["cost"]) + 1e-12   # R3 touches no goal: it does not move


def test_the_handle_after_the_call():
    """The handle's own values are untouched and its state is the state at entry: a plain run of the handle gives the bits it gave
    before the call from that state, which are also a fresh handle's."""
    from spicey_amd.lib import Handle, HipBackend
    seen = {}

    class Capture(HipBackend):
        def run_fit(self, flat, *args):
            seen["flat"], seen["args"] = flat, args
            return super().run_fit(flat, *args)

    start = parseNetlist(RC)
    start.C[0].vPrev = 0.75   # a state at entry that is not the zero state
    first = optimizeTRAN(start, MEASURES, GOALS, VARS, max_iter=3, backend=Capture())
    flat, (steps, dt, src, *rest) = seen["flat"], seen["args"]
    h, fresh = Handle(flat), Handle(flat)
    try:
        before = h.state()
        a0 = h.run(steps, dt, src, want_iters=False)   # the plain run before the call; it leaves its end state behind
        h.set_state(before)
        r = h.run_fit(steps, dt, src, *rest)
        after = h.state()
        a, b = h.run(steps, dt, src, want_iters=False), fresh.run(steps, dt, src, want_iters=False)
    finally:
        h.close()
        fresh.close()
    assert r["status"] == abi.OK and r["history"].shape == (3, 1, abi.FIT_ROW) and (r["n_iter"] == 3).all()
    assert (before["C_vprev"] == 0.75).all()
    for k in before:
        assert (np.asarray(before[k]).view(np.int64) == np.asarray(after[k]).view(np.int64)).all() if before[k].dtype == np.float64 else (before[k] == after[k]).all(), k
    for other in (a0, b):
        assert (a["out_v"].view(np.int64) == other["out_v"].view(np.int64)).all() and (a["out_i"].view(np.int64) == other["out_i"].view(np.int64)).all()
    assert a["status"] == abi.OK and a["out_v"][0, 0, 0] != 0.0   # (the run starts from the charged capacitor)
    assert [dict(zip(abi.FIT_ROW_KEYS, map(float, row[0]))) for row in r["history"]] == first["history"]
    # the refusals of the run: nothing runs
    bad = h_refusal(flat, steps, dt, src, rest)
    assert bad["status"] == abi.ERR_BAD_DESC and bad["detail"].startswith("fit: ") and "fourier" in bad["detail"]


def h_refusal(flat, steps, dt, src, rest):
    from spicey_amd.lib import Handle
    from spicey_amd.measure import make_four_reqs
    h = Handle(flat)
    try:
        req, act, step, g_lo, g_hi, g0, goals, scalars, reqs, treqs, preqs = rest
        wrong = abi.fit_req(2, len(act))
        r2 = h.run_fit(steps, dt, src, wrong, act, step, g_lo, g_hi, g0, goals, scalars, reqs, treqs, preqs)
        assert r2["status"] == abi.ERR_BAD_DESC and "instances" in r2["detail"] and r2["detail"].startswith("fit: ")
        none = abi.fit_req(1, len(act), max_iter=0)
        r3 = h.run_fit(steps, dt, src, none, act, step, g_lo, g_hi, g0, goals, scalars, reqs, treqs, preqs)
        assert r3["status"] == abi.ERR_BAD_DESC and r3["detail"] == "fit: max_iter must be >= 1"
        for bad in (0.0, -1.0, float("nan"), float("inf")):
            gb = np.array(g0, dtype=np.float64)
            gb[0, -1] = bad
            r4 = h.run_fit(steps, dt, src, req, act, step, g_lo, g_hi, gb, goals, scalars, reqs, treqs, preqs)
            assert r4["status"] == abi.ERR_BAD_DESC and r4["detail"] == "fit: a starting gain must be finite and > 0", r4["detail"]
        st = h.state()
        assert (st["C_vprev"] == 0.75).all()   # nothing ran
        return h.run_fit(steps, dt, src, req, act, step, g_lo, g_hi, g0, goals, scalars, reqs, treqs, preqs, freqs=make_four_reqs([(0, 0, -1, 3, 0, steps, 1e5)]))
    finally:
        h.close()


def test_a_structurally_singular_topology_gives_every_problem_status_2():
    """A switch whose control node hangs in the air: that node's row is empty.  As spicey_run_pss, the call reports it per problem —
    status 2, the starting values, an infinite cost — and raises nothing."""
    from spicey_amd.lib import HipBackend
    text = ".MODEL SWMOD SW\n" + RC.replace("R3 x 0 1000", "R3 x 0 1000\nS9 x 0 fc 0 SWMOD")
    r = optimizeTRAN(parseNetlist(text), MEASURES, GOALS, VARS, starts=[{}, {"R1": 1500.0}], max_iter=5, backend=HipBackend())
    print("iterations", [q["iterations"] for q in r["starts"]])
    assert [q["status"] for q in r["starts"]] == [abi.FIT_NOT_EVALUABLE] * 2 and not r["converged"] and r["cost"] == math.inf
    assert [q["values"] for q in r["starts"]] == [{"R1": 1000.0, "R2": 2000.0}, {"R1": 1500.0, "R2": 2000.0}]
    assert r["scalars"] == {"o.final": None, "o.avg": None} and all(q["iterations"] <= 1 for q in r["starts"])
