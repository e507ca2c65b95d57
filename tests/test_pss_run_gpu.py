"""steadyState / steadyStateBatch on the GPU (spicey_run_pss through HipBackend): every fixture converges within 12 iterations
to a state whose one-period residual ON THE CPU ORACLE is at most 2 and whose switch states return; the first iteration's row
equals the numpy update of the states read back around it bit for bit; a batch of load variants, one singular variant beside it;
measureTRAN from the written-back state.

The bound 2 is derived: 1 is the device's own stopping rule; 1 comes from the 1e-9 |v| + 1e-12 parity bar between the device's
and the oracle's transient, which at these tolerances (reltol 1e-6, abstol 1e-9 / 1e-12) is at most one tolerance unit.
Iteration counts are printed, and apart from the cap of 12 not asserted."""
import numpy as np
import pytest

import pss_cases as pc
from spicey_amd import abi, pss, steadyState, steadyStateBatch
from spicey_amd.measure import measureTRAN, stats
from spicey_amd.netlist import parseNetlist
from spicey_amd.simulate import SingularMatrixError

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", sorted(pc.NETLISTS))
def test_fixture_converges_on_the_device_to_a_fixed_point_of_the_oracle(name):
    from spicey_amd.lib import HipBackend
    ckt = parseNetlist(pc.NETLISTS[name])
    r = steadyState(ckt, max_iter=12, backend=HipBackend())
    res, on_back = pc.oracle_residual(pc.NETLISTS[name], r["state"])
    print(f"{name}: iterations {r['iterations']}, device residual {r['residual']:.3e}, oracle residual {res:.3e}, "
          f"pert switch diffs {[h['n_pert_switch_diff'] for h in r['history']]}")
    assert r["converged"] and r["status"] == 0 and r["iterations"] <= 12 and r["residual"] <= 1.0
    assert res <= 2.0 and on_back
    assert [e.vPrev for e in ckt.C] == list(r["state"]["C"].values())


@pytest.mark.parametrize("name", ["PSS_BOOST", "PSS_BUCK"])
def test_first_iteration_equals_the_numpy_update_of_the_states_around_it(name):
    from spicey_amd.lib import Handle
    ckt = parseNetlist(pc.NETLISTS[name])
    dt, _ = abi.computeEffectiveTimeStep(ckt.analyses["tran"]["dt"], ckt.analyses["tran"]["tstop"])
    m = pc.STEPS_PER_PERIOD[name]
    src = pss.period_table(ckt, dt, m)
    one = abi.flatten(ckt)
    one.out_nodes = np.array([1], np.int32)
    kinds = (one.nC, one.nL, one.nD)
    nX = sum(kinds)
    W = 1 + nX
    # a start away from zero, different per circuit
    n_ckt = 2
    rng = np.random.default_rng(7)
    flat = abi.stack_instances([one.replicate(W) for _ in range(n_ckt)])
    base = rng.uniform(0.1, 1.0, (n_ckt, nX))
    start = np.repeat(base, W, axis=0)
    flat.C_vprev[:], flat.L_iprev[:], flat.D_vdprev[:] = start[:, :one.nC], start[:, one.nC:one.nC + one.nL], start[:, one.nC + one.nL:]
    req = abi.pss_req(n_ckt, max_iter=1)
    h = Handle(flat)
    try:
        before = h.state()
        r = h.run_pss(m, dt, src, req)
        after = h.state()
    finally:
        h.close()
    assert r["status"] == abi.OK, r["detail"]
    b0, on0 = pss.state_matrix(before)[::W], before["S_ison"][::W]
    assert (b0.view(np.int64) == base.view(np.int64)).all()
    # the same design on a second handle, one plain run, the end states back: the numpy update of them is the device's row
    X, on, hh = pss.design_reference_pss(b0, on0, kinds, abi.PSS_NEWTON, req.rel_step, req.v_scale, req.i_scale)
    h2 = Handle(pss._with_state(flat, X, on))
    try:
        res = h2.run(m - 1, dt, src, want_currents=False, want_iters=False)
    finally:
        h2.close()
    assert res["status"] == abi.OK, res["detail"]
    nb, nbon, delta, rows, done = pss.reduce_reference_pss(b0, on0, hh, pss.state_matrix(res["state"]), res["state"]["S_ison"], np.zeros(n_ckt, np.int32), kinds)
    assert r["history"].shape == (1, n_ckt, abi.PSS_ROW)
    assert (r["history"][0].view(np.int64) == rows.view(np.int64)).all(), (r["history"][0], rows)
    assert (r["x"].view(np.int64) == nb.view(np.int64)).all() and (r["on"] == nbon).all()
    assert (r["n_iter"] == 1).all() and (r["ckt_status"] == np.where(done == 1, 0, 1)).all()
    # on return every instance of a circuit holds the new base
    assert (pss.state_matrix(after).view(np.int64) == np.repeat(nb, W, axis=0).view(np.int64)).all() and (after["S_ison"] == np.repeat(nbon, W, axis=0)).all()
    assert r["pss_ms"] > 0.0 and r["tran_ms"] > 0.0


def test_batch_of_load_variants_and_a_singular_one_beside_them():
    from spicey_amd.lib import HipBackend
    texts = [pc.boost(r1) for r1 in ("50", "100", "200")]
    out = steadyStateBatch([parseNetlist(t) for t in texts], max_iter=12, backend=HipBackend())
    for r, text in zip(out, texts):
        res, on_back = pc.oracle_residual(text, r["state"])
        print(f"batch slot: iterations {r['iterations']}, oracle residual {res:.3e}")
        assert r["converged"] and res <= 2.0 and on_back
    assert len({r["state"]["C"]["C1"] for r in out}) == 3
    # a switch whose control node hangs in the air: that node's row is empty, the matrix singular by its structure
    bad = pc.boost("100").replace("R1 n3 0 100", "R1 n3 0 100\nS9 n3 0 fc 0 SWMOD")
    ckts = [parseNetlist(t) for t in texts] + [parseNetlist(bad)]
    out = steadyStateBatch(ckts, max_iter=12, backend=HipBackend())
    assert isinstance(out[3], SingularMatrixError) and all(e.vPrev == 0.0 for e in ckts[3].C)
    for r, text in zip(out[:3], texts):
        res, on_back = pc.oracle_residual(text, r["state"])
        assert r["converged"] and res <= 2.0 and on_back


def test_measure_tran_from_the_written_back_state_sees_identical_periods():
    from spicey_amd.lib import HipBackend
    ckt = parseNetlist(pc.NETLISTS["PSS_BOOST"])
    r = steadyState(ckt, max_iter=12, backend=HipBackend())
    assert r["converged"]
    m, T = r["steps_per_period"], r["period"]
    dt = T / m
    ckt.analyses["tran"] = {"dt": dt, "tstop": (3 * m - 1) * dt}
    assert abi.computeEffectiveTimeStep(dt, (3 * m - 1) * dt)[1] == 3 * m - 1
    got = measureTRAN(ckt, {"all": stats("v(n3)"), "last": stats("v(n3)", t_from=2 * m * dt)}, backend=HipBackend())
    unit = pc.RELTOL * abs(got["all"]["max"]) + pc.VABSTOL
    print("pp over 3 periods", got["all"]["pp"], "pp of the last", got["last"]["pp"], "in tolerance units", abs(got["all"]["pp"] - got["last"]["pp"]) / unit)
    assert abs(got["all"]["pp"] - got["last"]["pp"]) <= 2.0 * unit


@pytest.mark.parametrize("name", ["PSS_BOOST", "PSS_BUCK"])
def test_the_reference_order_engine_is_served_and_lands_where_the_oracle_does(name):
    """spicey_run_pss serves every engine that starts from and ends in the handle's state.  The reference-order engine gives the
    oracle's transient bit for bit, so the whole iteration equals the host loop over the oracle: the same rows, the same state."""
    from oracle.pyoracle import OracleBackend
    from spicey_amd.lib import HipBackend
    r = steadyState(parseNetlist(pc.NETLISTS[name]), max_iter=12, backend=HipBackend(interpreter=3))
    ref = steadyState(parseNetlist(pc.NETLISTS[name]), max_iter=12, backend=OracleBackend())
    assert r["converged"] and r["iterations"] == ref["iterations"]
    assert r["history"] == ref["history"] and r["state"] == ref["state"]
