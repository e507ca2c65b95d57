"""optimizeTRAN / optimizeTRANBatch without a GPU: goal and variable parsing, the refusals, the seeded starts, and host_run_fit on
the CPU oracle backend for a two-element RC problem — the returned circuit, simulated by the oracle and evaluated by the numpy
measure reference, satisfies the goals to the stopping rule."""
import math

import numpy as np
import pytest

from oracle.pyoracle import OracleBackend
from spicey_amd import abi, fit, optimizeTRAN, optimizeTRANBatch
from spicey_amd.fit import at_least, at_most, between, target
from spicey_amd.measure import fourier, measureTRAN, stats
from spicey_amd.netlist import parseNetlist

# a loaded RC low-pass behind a 5 V step from the zero state: v(out) settles to 5 R2 / (R1 + R2) with tau = (R1 || R2) C1
RC = "V1 in 0 5\nR1 in out 1000\nC1 out 0 2e-9\nR2 out 0 2000\n.tran 4e-7 4e-5\n.end\n"
MEASURES = {"o": stats("v(out)")}
# two equalities pin the two variables — the divider pins R1, the average pins the time constant and with it C1 — and a ceiling
# that the output never reaches stays an inactive, zero row: the residuals are smooth in the gains and vanish at the solution
GOALS = {"o.final": target(3.0, scale=0.01), "o.avg": target(2.7, scale=0.01), "o.max": at_most(3.5, scale=0.01)}
VARS = {"R1": (200.0, 5000.0), "C1": (5e-10, 5e-8)}


def test_goal_records():
    assert target(5.0) == ("goal", abi.FIT_EQ, 5.0, 5.0, 0.2) and target(0.0)[4] == 1.0 / fit.TINY
    assert at_most(0.03, scale=0.01) == ("goal", abi.FIT_AT_MOST, 0.0, 0.03, 100.0) and at_least(-2.0) == ("goal", abi.FIT_AT_LEAST, -2.0, 0.0, 0.5)
    assert between(1.0, 4.0) == ("goal", abi.FIT_BETWEEN, 1.0, 4.0, 0.25)
    for bad in (lambda: target(float("nan")), lambda: at_most(1.0, scale=0.0), lambda: between(2.0, 1.0), lambda: target(True), lambda: at_least(1.0, scale=float("inf"))):
        with pytest.raises(ValueError, match="optimizeTRAN"):
            bad()
    rec = abi.fit_goals([g[1:] for g in (target(5.0), at_most(0.03, scale=0.01))])
    assert rec.dtype == abi.FIT_GOAL_DTYPE and rec["kind"].tolist() == [0, 1] and rec["weight"].tolist() == [0.2, 100.0] and rec["pad"].tolist() == [0, 0]


def test_variables_become_gains_on_the_circuits_values():
    ckt = parseNetlist(RC)
    elements, act, lo, hi = fit._resolve_vars(ckt, {"c1": (1e-9, 4e-9), "R1": (500.0, 2000.0)})
    assert act.tolist() == [0, 2] and [elements[e][0] for e in act] == ["R1", "C1"]   # ascending in the order R, C, L
    assert lo.tolist() == [500.0 / 1000.0, 1e-9 / 2e-9] and hi.tolist() == [2000.0 / 1000.0, 4e-9 / 2e-9]


def test_refusals():
    ckt = parseNetlist(RC)
    be = OracleBackend()

    def refused(text, exc=ValueError, measures=MEASURES, goals=GOALS, vars=VARS, **kw):
        with pytest.raises(exc) as e:
            optimizeTRAN(ckt, measures, goals, vars, backend=be, **kw)
        assert "optimizeTRAN" in str(e.value) and text in str(e.value), str(e.value)

    refused("no R, C or L", vars={"L9": (1.0, 2.0)})                                   # an unknown element
    refused("do not contain the circuit's own value", vars={"R1": (2000.0, 5000.0)})     # no start is given
    refused("root field", goals={"o.rms": target(3.0)})
    refused("square the target", goals={"o.rms": target(3.0)})
    refused("no measure defines", goals={"o.median": target(3.0)})
    refused("no measure defines", goals={"x.final": target(3.0)})
    refused("only a root field", goals={"o.final^2": target(9.0)})
    refused("no goals", goals={})
    refused("no variables", vars={})
    refused("0 < low <= high", vars={"R1": (0.0, 10.0)})
    refused("(low, high)", vars={"R1": 5.0})
    refused("target(...)", goals={"o.final": 3.0})
    refused("outside the bounds", starts=[{"R1": 100.0}])
    refused("no variable", starts=[{"R2": 100.0}])
    refused("rel_step", rel_step=1.0)
    refused("not reduced across instances", exc=TypeError, measures={"f": fourier("v(out)", 1e5)})
    assert optimizeTRAN(parseNetlist(RC.replace(".tran 4e-7 4e-5\n", "")), MEASURES, GOALS, VARS, backend=be) is None
    # a start inside the bounds lifts the second refusal
    ckt2 = parseNetlist(RC)
    elements, act, lo, hi = fit._resolve_vars(ckt2, {"R1": (2000.0, 5000.0)})
    assert fit._starts([{"R1": 2500.0}], 0, elements, act, lo, hi).tolist() == [[2.5]]


def test_starts_are_deterministic_in_the_seed():
    ckt = parseNetlist(RC)
    elements, act, lo, hi = fit._resolve_vars(ckt, VARS)
    a, b, c = (fit._starts(5, seed, elements, act, lo, hi) for seed in (3, 3, 4))
    assert a.shape == (5, 2) and (a.view(np.int64) == b.view(np.int64)).all() and (a[1:] != c[1:]).any()
    assert (a[0] == 1.0).all() and (a >= lo).all() and (a <= hi).all()   # the circuit's own values first
    assert fit._starts(None, 0, elements, act, lo, hi).tolist() == [[1.0, 1.0]]
    with pytest.raises(ValueError, match="starts must be >= 1"):
        fit._starts(0, 0, elements, act, lo, hi)


def _residuals(goals, scalars):
    out = {}
    for key, (_, kind, lo, hi, w) in goals.items():
        x = scalars[key]
        out[key] = w * (x - lo) if kind == abi.FIT_EQ else w * (x - hi) if kind != abi.FIT_AT_LEAST and x > hi else w * (x - lo) if kind != abi.FIT_AT_MOST and x < lo else 0.0
    return out


_RESULT = {}


def _solved():
    if not _RESULT:
        ckt = parseNetlist(RC)
        _RESULT["ckt"] = ckt
        _RESULT["r"] = optimizeTRAN(ckt, MEASURES, GOALS, VARS, max_iter=30, backend=OracleBackend())
    return _RESULT["ckt"], _RESULT["r"]


def test_host_loop_on_the_oracle_meets_the_goals_to_the_stopping_rule():
    ckt, r = _solved()
    print("iterations", r["iterations"], "cost", r["cost"], "values", r["values"], "scalars", r["scalars"], "lambda", [h["lambda"] for h in r["history"]])
    assert r["converged"] and r["status"] == 0 and 1 <= r["iterations"] <= 30 and len(r["history"]) == r["iterations"] and r["history"][-1]["status"] == 0.0
    # the input circuit is not mutated; the copy holds the values
    assert (ckt.R[0].R, ckt.C[0].C, ckt.R[1].R) == (1000.0, 2e-9, 2000.0)
    out = r["circuit"]
    assert out is not ckt and (out.R[0].R, out.C[0].C, out.R[1].R) == (r["values"]["R1"], r["values"]["C1"], 2000.0)
    assert VARS["R1"][0] <= r["values"]["R1"] <= VARS["R1"][1] and VARS["C1"][0] <= r["values"]["C1"] <= VARS["C1"][1]
    # the oracle's simulation of the returned circuit, evaluated by the numpy measure reference: the same scalars, bit for bit —
    # the gains that come back belong to a point that was evaluated — and the stopping rule on them
    got = measureTRAN(out, MEASURES, backend=OracleBackend())["o"]
    assert {"o.final": got["final"], "o.avg": got["avg"], "o.max": got["max"]} == r["scalars"]
    res = _residuals(GOALS, r["scalars"])
    F = 0.0
    for v in res.values():
        F = F + v * v
    last = r["history"][-1]
    assert F == r["cost"] == last["F_good"] and (F <= 1e-6 or last["max_step"] <= 1e-6)
    # the goals themselves: each equality to its scale times sqrt(F), the ceiling met
    assert abs(got["final"] - 3.0) <= 0.01 * math.sqrt(F) and abs(got["avg"] - 2.7) <= 0.01 * math.sqrt(F) and got["max"] <= 3.5 and res["o.max"] == 0.0
    assert F <= 1e-6   # (a smooth problem with a zero-residual solution: Gauss-Newton's last steps square the residual; 1e-6 is 1e-3 of a scale unit)
    # R1 follows from the divider alone: 5 R2 / (R1 + R2) = 3 once the output has settled (tau << the run)
    assert abs(r["values"]["R1"] - 4000.0 / 3.0) <= 1e-3 * 4000.0 / 3.0


def test_starts_run_as_further_circuits_and_the_batch_is_one_handle():
    calls = []

    class Counting(OracleBackend):
        def run(self, flat, *a, **k):
            calls.append(flat.n_inst)
            return super().run(flat, *a, **k)

    r = optimizeTRAN(parseNetlist(RC), MEASURES, GOALS, VARS, starts=3, seed=1, max_iter=30, backend=Counting())
    assert len(r["starts"]) == 3 and set(calls) == {3 * 5} and len(calls) == max(s["iterations"] for s in r["starts"])
    assert r["best_start"] == min((s for s in range(3) if r["starts"][s]["converged"]), key=lambda s: (r["starts"][s]["cost"], s)) and r["converged"]
    # start 0 is the plain run, bit for bit: the problems of one handle are independent
    _, one = _solved()
    assert r["starts"][0]["values"] == one["values"] and r["starts"][0]["history"] == one["history"]
    # a batch of two load variants: one problem per circuit
    a, b = optimizeTRANBatch([parseNetlist(RC), parseNetlist(RC.replace("R2 out 0 2000", "R2 out 0 3000"))], MEASURES, GOALS, VARS, backend=OracleBackend())
    assert a["values"] == one["values"] and b["converged"] and abs(b["values"]["R1"] - 2000.0) <= 1e-3 * 2000.0
