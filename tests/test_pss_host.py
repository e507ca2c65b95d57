"""The periodic steady state without a GPU: the design and the Newton update of pss_exec.h through the CPU harness
(tests/pss_host) against their numpy restatements (spicey_amd/pss.py) bit for bit — delta, the new base, base_on, done and all 8
row fields —, delta against numpy.linalg.solve within the forward bound of two pivoted eliminations, small cases in dyadic numbers
whose answer is exact, and the refusals of the judge.  `make asan` in tests/pss_host builds and runs the same code as a
stand-alone program under the address and undefined-behaviour sanitizers (not part of the suite)."""
import numpy as np
import pytest

from pss_host import pypss as pp
from spicey_amd import abi, pss


def _same(got, ref, what):
    for g, r, name in zip(got, ref, ("base", "base_on", "delta", "rows", "done")):
        assert g.shape == r.shape, (what, name)
        same = pp.bits_equal(g, r) if g.dtype == np.float64 else g == r
        assert same.all(), (what, name, g, r)


@pytest.mark.parametrize("nX", pp.NX)
def test_design_equals_numpy_bit_for_bit(nX):
    for n_ckt in pp.NCKT:
        kinds, req, base, base_on, h, *_ = pp.linear_case(nX, n_ckt, seed=nX)
        base[0, 0] = 0.0   # |base| below the scale: the step is the scale's
        if base.size > 1:
            base[-1, -1] = -123.5
        X, on, hh = pp.design(kinds, req, base, base_on)
        rX, ron, rh = pss.design_reference_pss(base, base_on, kinds, abi.PSS_NEWTON, req.rel_step, req.v_scale, req.i_scale)
        assert pp.bits_equal(X, rX).all() and (on == ron).all() and pp.bits_equal(hh, rh).all()
        W = 1 + nX
        moved = X.reshape(n_ckt, W, nX) != base[:, None, :]
        assert (moved[:, 0] == 0).all() and (moved[:, 1:] == np.eye(nX, dtype=bool)[None]).all()
        assert (hh > 0).all() and hh[0, 0] == req.rel_step * req.v_scale
        # no perturbation: every instance holds the base, h is left alone
        X0, on0, h0 = pp.design(kinds, req, base, base_on, perturb=False)
        assert pp.bits_equal(X0.reshape(n_ckt, W, nX), np.broadcast_to(base[:, None, :], (n_ckt, W, nX))).all() and (on0 == ron).all() and (h0 == pp.SENTINEL).all()
    # settle: one instance per circuit
    req = abi.pss_req(2, abi.PSS_SETTLE)
    Xs, ons, hs = pp.design((2, 1, 0), req, [[1.0, 2.0, 3.0], [4.0, 5.0, 6.0]], [[1], [0]])
    assert Xs.tolist() == [[1.0, 2.0, 3.0], [4.0, 5.0, 6.0]] and ons.tolist() == [[1], [0]] and (hs == pp.SENTINEL).all()


@pytest.mark.parametrize("n_ckt", pp.NCKT)
@pytest.mark.parametrize("nX", pp.NX)
def test_update_equals_numpy_bit_for_bit_and_solves_the_system(nX, n_ckt):
    """Seeded J with |J_ia| <= 0.9 / nX: M = I - J is strictly diagonally dominant, cond_inf(M) <= 19.  delta agrees with
    numpy.linalg.solve to 2 * 19 * nX * 2^-52 * |delta|_inf: two pivoted eliminations, each inside the forward bound with growth
    <= 2 (derived, not tuned)."""
    kinds, req, base, base_on, h, X, on, done, J = pp.linear_case(nX, n_ckt, seed=100 * nX + n_ckt)
    got = pp.update(kinds, req, base, base_on, h, X, on, done)
    ref = pp.reference_update(kinds, req, base, base_on, h, X, on, done)
    _same(got, ref, (nX, n_ckt))
    for threads in (64, 192):  # nothing depends on the workgroup's size
        _same(pp.update(kinds, req, base, base_on, h, X, on, done, threads=threads), got, (nX, n_ckt, threads))
    nb, nbon, delta, rows, ndone = got
    M, r = pp.fd_matrix(base, h, X)
    W = 1 + nX
    for c in range(n_ckt):
        assert np.linalg.cond(M[c], np.inf) <= 19.0
        want = np.linalg.solve(M[c], r[c])
        bound = 2 * 19 * nX * 2.0 ** -52 * np.abs(want).max()
        err = np.abs(delta[c] - want).max()
        print(f"nX={nX} c={c}: |delta - solve|_inf = {err:.3e}, bound {bound:.3e}")
        assert err <= bound
        assert rows[c, 3] == 1.0 and rows[c, 7] == 0.0 and ndone[c] == 0 and rows[c, 2] == 1.0 and rows[c, 6] == (1.0 if nX > 1 else 0.0)
        assert pp.bits_equal(nb[c], base[c] + delta[c]).all() and (nbon[c] == on.reshape(n_ckt, W, -1)[c, 0]).all()
        assert 0.1 <= rows[c, 5] <= 1.9


def _run_exact(name, update=pp.update):
    k = pp.exact_case(name)
    got = update(k["kinds"], k["req"], k["base"], k["base_on"], k["h"], k["X"], k["on"], k["done"], k["ist"])
    ref = pp.reference_update(k["kinds"], k["req"], k["base"], k["base_on"], k["h"], k["X"], k["on"], k["done"], k["ist"])
    return k, got, ref


def check_exact(name, k, got):
    """What is known exactly of a named case."""
    nb, nbon, delta, rows, done = got
    e = k["expect"]
    if "status" in e:
        assert rows[:, 3].tolist() == e["status"], name
        assert done.tolist() == [1 if k["done"][c] else (0 if s == 1 else 1 if s == 0 else int(s)) for c, s in enumerate(e["status"])], name
    if "delta" in e:
        assert (delta == np.asarray(e["delta"])).all(), (name, delta)
    if "base" in e:
        assert (nb == np.asarray(e["base"])).all(), (name, nb)
    if e.get("base_unchanged"):
        assert pp.bits_equal(nb, k["base"]).all() and (nbon == k["base_on"]).all() and (delta == pp.SENTINEL).all(), name
    if "min_pivot" in e:
        assert rows[:, 5].tolist() == e["min_pivot"], (name, rows)
    if "n_switch_mismatch" in e:
        assert rows[:, 2].tolist() == e["n_switch_mismatch"] and (nbon == k["on"][:1]).all(), name
    if name == "converged":
        assert rows[0].tolist() == [0.0, 0.0, 0.0, 0.0, 0.0, -1.0, 0.0, 1.0]
    if name == "done_beside":
        assert pp.bits_equal(nb[0], k["base"][0]).all() and (rows[0] == pp.SENTINEL).all() and (nb[1] == k["base"][1] + delta[1]).all()
    if name == "damping":
        assert (nb == k["base"] + 0.5 * delta).all()
    if name == "settle":
        assert rows[0, 1] == np.abs(delta[0] / (k["req"].reltol * np.abs(k["base"][0]) + k["req"].vabstol)).max() and rows[0, 5] == -1.0


@pytest.mark.parametrize("name", [n for n in pp.EXACT if n != "h_representable"])
def test_exact_small_cases(name):
    k, got, ref = _run_exact(name)
    _same(got, ref, name)
    check_exact(name, k, got)
    if k["expect"].get("status") == [1] and "delta" in k["expect"] and k["h"] is not None:
        M, r = pp.fd_matrix(k["base"], k["h"], k["X"])
        assert (M[0] @ got[2][0] == r[0]).all()  # dyadic numbers: the product is exact


def test_h_eff_is_the_representable_difference():
    k = pp.exact_case("h_representable")
    X, on, h = pp.design(k["kinds"], k["req"], k["base"], k["base_on"])
    step = k["req"].rel_step * np.maximum(np.abs(k["base"]), 1.0)
    assert pp.bits_equal(h, k["expect"]["h"]).all() and (h != step).any()
    assert pp.bits_equal(h[0], np.array([X[1, 0], X[2, 1]]) - k["base"][0]).all()


def test_refusals():
    kinds, req, base, base_on, h, X, on, done, _ = pp.linear_case(3, 1, seed=1)

    def refused(text, kinds=kinds, req=req, base=base, h=h, X=X, **kw):
        for call in (lambda: pp.update(kinds, req, base, base_on, h, X, on, done, **kw), lambda: pp.design(kinds, req, base, base_on, **kw)):
            with pytest.raises(pp.Refused) as e:
                call()
            assert str(e.value).startswith("pss: ") and text in str(e.value), str(e.value)

    big = np.zeros((1, 129))
    refused('method = "settle"', kinds=(129, 0, 0), base=big, h=big, X=np.zeros((130, 129)))
    refused("no state", kinds=(0, 0, 0), base=np.zeros((1, 0)), h=None, X=np.zeros((1, 0)))
    refused("null request", req=None)
    refused("workspace too small", work_bytes=8)
    refused("null buffer", have_work=False)
    for field, bad, text in (("struct_bytes", 80, "struct_bytes"), ("reserved", 1, "reserved"), ("pad", 1, "reserved"), ("method", 2, "unknown method"),
                             ("n_ckt", 0, "n_ckt"), ("reltol", 0.0, "tolerances"), ("vabstol", -1.0, "tolerances"), ("iabstol", float("nan"), "tolerances"),
                             ("rel_step", 0.0, "rel_step"), ("v_scale", float("inf"), "rel_step"), ("i_scale", 0.0, "rel_step"), ("damping", 0.0, "damping"),
                             ("damping", 1.5, "damping")):
        r = abi.pss_req(1)
        setattr(r, field, bad)
        refused(text, req=r)
    with pytest.raises(pp.Refused):
        pp.update(kinds, req, base, base_on, None, X, on, done)
    # 129 states settle
    reqs = abi.pss_req(1, abi.PSS_SETTLE)
    nb, _, _, rows, _ = pp.update((129, 0, 0), reqs, big, np.zeros((1, 0), np.int32), None, np.ones((1, 129)), np.zeros((1, 0), np.int32), [0])
    assert (nb == 1.0).all() and rows[0, 3] == 1.0
    assert pp.lib().spicey_pss_host_workspace_bytes(1, 129, abi.PSS_NEWTON) == -1 and pp.lib().spicey_pss_host_workspace_bytes(1, 129, abi.PSS_SETTLE) > 0
    assert pp.lib().spicey_pss_host_lds_bytes(abi.PSS_NEWTON, 128) == 132096
