"""The element sizing without a GPU: the design and the damped least-squares update of fit_exec.h through the CPU harness
(tests/fit_host) against their numpy restatements (spicey_amd/fit.py) bit for bit — the gains, all 8 row fields, done and the
circuits' state (A, b, g_good, F_good, lambda) —, small cases in representable numbers whose step is written down, not computed,
and the refusals of the judge.  `make asan` in tests/fit_host builds and runs the same code as a stand-alone program under the
address and undefined-behaviour sanitizers (not part of the suite)."""
import numpy as np
import pytest

from fit_host import pyfit as pf
from spicey_amd import abi, fit


def _same(got, ref, what):
    for g, r, name in zip(got, ref, ("g", "rows", "done", "state")):
        assert g.shape == r.shape, (what, name)
        same = pf.bits_equal(g, r) if g.dtype == np.float64 else g == r
        assert same.all(), (what, name, g, r)


@pytest.mark.parametrize("nA", pf.NA)
def test_design_equals_numpy_bit_for_bit(nA):
    for n_ckt in pf.NCKT:
        rng = np.random.default_rng(10 * nA + n_ckt)
        W = 1 + 2 * nA
        ni = n_ckt * W
        kinds = ((nA + 2) // 3 + 1, (nA + 1) // 3 + 1, nA // 3 + 2)   # more elements than active ones, every kind present
        nE = sum(kinds)
        R, Cv, Lv = (rng.uniform(0.5, 2.0, (ni, k)) * 10.0 ** rng.integers(-9, 4) for k in kinds)
        act = np.sort(rng.choice(nE, nA, replace=False)).astype(np.int32)
        step = rng.choice([1e-3, 2.0 ** -9, 5e-4], nA)
        g = rng.uniform(0.3, 3.0, (n_ckt, nA))
        req = abi.fit_req(n_ckt, nA)
        got = pf.design(kinds, R, Cv, Lv, req, act, step, g)
        ref = fit.design_reference_fit(R, Cv, Lv, act, step, g)
        for a, b in zip(got, ref):
            assert pf.bits_equal(a, b).all(), (nA, n_ckt)
        v, o = np.concatenate([R, Cv, Lv], axis=1).reshape(n_ckt, W, nE), np.concatenate(got, axis=1).reshape(n_ckt, W, nE)
        inactive = np.setdiff1d(np.arange(nE), act)
        assert pf.bits_equal(o[:, :, inactive], v[:, :, inactive]).all()
        assert pf.bits_equal(o[:, 0, act], v[:, 0, act] * g).all()
        for a in (0, nA - 1):   # the perturbed pair of an element: its own gain alone moves
            assert pf.bits_equal(o[:, 1 + 2 * a, act[a]], v[:, 1 + 2 * a, act[a]] * (g[:, a] * (1.0 + step[a]))).all()
            assert pf.bits_equal(o[:, 2 + 2 * a, act[a]], v[:, 2 + 2 * a, act[a]] * (g[:, a] * (1.0 - step[a]))).all()
            other = np.setdiff1d(np.arange(nA), [a])
            assert pf.bits_equal(o[:, 1 + 2 * a, act[other]], v[:, 1 + 2 * a, act[other]] * g[:, other]).all()


@pytest.mark.parametrize("n_scalar", pf.NSCALAR)
@pytest.mark.parametrize("nA", pf.NA)
def test_update_equals_numpy_bit_for_bit(nA, n_scalar):
    """An accepted first update, then — on the same workspace — a second one with other scalars (accepted or rejected as the
    numbers fall): both equal numpy, and nothing depends on the workgroup's size."""
    for n_ckt in pf.NCKT:
        req, step, g_lo, g_hi, goals, x, g, done = pf.random_case(nA, n_scalar, n_ckt, seed=1000 * nA + 10 * n_scalar + n_ckt)
        work = pf.workspace(n_ckt, nA, n_scalar)
        got = pf.update(req, True, step, g_lo, g_hi, goals, None, x, g, done, work)
        ref = pf.reference_update(req, True, step, g_lo, g_hi, goals, None, x, g, done)
        _same(got, ref, (nA, n_scalar, n_ckt, "first"))
        assert (got[1][:, 3] == 1.0).all() and (got[1][:, 4] == 1.0).all() and (got[1][:, 6] == 0.0).all()
        if nA in (5, 65):
            for threads in (64, 192):
                _same(pf.update(req, True, step, g_lo, g_hi, goals, None, x, g, done, threads=threads), got, (nA, n_scalar, n_ckt, threads))
        # the second update: circuits 0 and 1 see a lower cost (x_0 moved halfway to its target), circuit 1 with a NaN in a perturbed
        # instance (that column is frozen); circuit 2 has an invalid instance and the cost it had: the same cost is not a lower one
        x2 = x.copy()
        W = 1 + 2 * nA
        valid = None
        for c in range(min(n_ckt, 2)):
            x2[c * W:(c + 1) * W, 0] = 0.5 * (x[c * W:(c + 1) * W, 0] + goals[c, 0]["lo"])
        if n_ckt > 1:
            x2[W + 1, 0] = np.nan
            valid = np.ones(n_ckt * W, np.uint8)
            valid[2 * W + 2 * nA] = 0
        got2 = pf.update(req, False, step, g_lo, g_hi, goals, valid, x2, got[0], got[2], work, rows=got[1])
        ref2 = pf.reference_update(req, False, step, g_lo, g_hi, goals, valid, x2, ref[0], ref[2], ref[3], ref[1])
        _same(got2, ref2, (nA, n_scalar, n_ckt, "second"))
        assert got2[1][0, 3] == 1.0 and got2[1][0, 0] < got[1][0, 0] and got2[1][0, 2] == got[1][0, 2] * req.lam_down
        if n_ckt > 1:
            assert got2[1][1, 3] == 1.0 and got2[1][1, 6] == 1.0
            assert got2[1][2, 3] == 0.0 and got2[1][2, 2] == got[1][2, 2] * req.lam_up and got2[1][2, 1] == got[1][2, 1]


def run_exact(name, update=pf.update):
    """[(g, rows, done, state)] per call of a named case, on one workspace."""
    k = pf.exact_case(name)
    n_ckt, ns = k["g"].shape[0], k["goals"].shape[1]
    work = update.new_work(n_ckt, 2, ns) if hasattr(update, "new_work") else pf.workspace(n_ckt, 2, ns)
    g, done, rows, out = k["g"], k["done"], None, []
    for call in k["calls"]:
        got = update(k["req"], call["first"], k["step"], k["g_lo"], k["g_hi"], k["goals"], call["valid"], call["x"], g, done, work, rows=rows)
        out.append(got)
        g, rows, done = got[0], got[1], got[2]
    return k, out


def reference_exact(k):
    g, done, rows, state, out = k["g"], k["done"], None, None, []
    for call in k["calls"]:
        got = pf.reference_update(k["req"], call["first"], k["step"], k["g_lo"], k["g_hi"], k["goals"], call["valid"], call["x"], g, done, state, rows)
        out.append(got)
        g, rows, done, state = got
    return out


def check_exact(name, k, out):
    """What is known exactly of a named case."""
    for n, (e, (g, rows, done, state)) in enumerate(zip(k["expect"], out)):
        what = (name, n, rows, g)
        status = e["status"] if isinstance(e["status"], list) else [e["status"]]
        assert rows[:, 4].tolist() == [float(s) for s in status], what
        if "g" in e:
            assert (g == np.asarray(e["g"])).all(), what
        if "close_g" in e:
            assert np.allclose(g, e["close_g"], rtol=1e-15, atol=0.0), what
        for key, col in (("F", 0), ("F_good", 1), ("lam", 2), ("accepted", 3), ("d", 5), ("n_frozen", 6), ("n_clamped", 7)):
            if key in e:
                assert rows[0, col] == e[key], (what, key)
        if "g_good" in e:
            assert (state[0, 6:8] == np.asarray(e["g_good"])).all(), what
        if "done" in e:
            assert done.tolist() == [e["done"]], what
    if name == "done_beside":
        assert (out[0][1][0] == pf.SENTINEL).all() and out[0][2].tolist() == [1, 0] and (out[0][3][0] == 0.0).all()
    if name in ("reject", "stall"):
        # the saved normal equations are the first call's, bit for bit
        assert pf.bits_equal(out[1][3][0, :6], out[0][3][0, :6]).all() and out[0][3][0, :6].tolist() == [4.0, 0.0, 0.0, 16.0, -1.0, 4.0]
    if name == "nan_column":
        assert out[0][3][0, :6].tolist() == [4.0, 0.0, 0.0, 0.0, -1.0, 0.0]
    if name == "invalid_first":
        assert (out[0][3] == 0.0).all()   # nothing was saved


@pytest.mark.parametrize("name", pf.EXACT)
def test_exact_small_cases(name):
    k, out = run_exact(name)
    for n, (got, ref) in enumerate(zip(out, reference_exact(k))):
        _same(got, ref, (name, n))
    check_exact(name, k, out)


def test_a_done_circuit_is_not_touched_by_later_updates():
    k, out = run_exact("stall")
    g, rows, done, state = out[-1]
    again = pf.update(k["req"], False, k["step"], k["g_lo"], k["g_hi"], k["goals"], None, k["calls"][0]["x"], g, done, rows=rows)
    assert pf.bits_equal(again[0], g).all() and pf.bits_equal(again[1], rows).all() and again[2].tolist() == [5]


def test_refusals():
    req, step, g_lo, g_hi, goals, x, g, done = pf.random_case(3, 2, 1, seed=1)
    R = np.ones((7, 4))
    Z = np.zeros((7, 0))
    act = np.array([0, 1, 3], np.int32)

    def refused(text, design=True, update=True, **kw):
        a = dict(req=req, step=step, g_lo=g_lo, g_hi=g_hi, goals=goals, x=x, g=g, act=act)
        a.update({k: v for k, v in kw.items() if k in a})
        extra = {k: v for k, v in kw.items() if k not in a}
        calls = []
        if update:
            calls.append(lambda: pf.update(a["req"], True, a["step"], a["g_lo"], a["g_hi"], a["goals"], None, a["x"], a["g"], done,
                                           **{k: v for k, v in extra.items() if k in ("work", "have_work", "n_scalar")}))
        if design:
            calls.append(lambda: pf.design((4, 0, 0), R, Z, Z, a["req"], a["act"], a["step"], a["g"], **{k: v for k, v in extra.items() if k in ("work", "have_work")}))
        for call in calls:
            with pytest.raises(pf.Refused) as e:
                call()
            assert str(e.value).startswith("fit: ") and text in str(e.value), str(e.value)

    refused("null request", req=None)
    refused("workspace too small", work=np.zeros(8, np.uint8))
    refused("null buffer", have_work=False)
    for field, bad, text in (("struct_bytes", 88, "struct_bytes"), ("reserved", 1, "reserved"), ("pad", 1, "reserved"), ("n_ckt", 0, "n_ckt"), ("nA", 0, "nA >= 1"),
                             ("nA", 129, "128"), ("lambda0", -1.0, "lambda0"), ("lambda0", float("nan"), "lambda0"), ("lam_up", 1.0, "lam_up"),
                             ("lam_down", 0.0, "lam_down"), ("lam_down", 1.5, "lam_down"), ("lam_max", float("inf"), "lam_max"), ("max_step", 0.0, "max_step"),
                             ("x_tol", -1.0, "x_tol"), ("f_tol", float("nan"), "x_tol"), ("pivot_min", 0.0, "pivot_min")):
        r = abi.fit_req(1, 3)
        setattr(r, field, bad)
        refused(text, req=r)
    r = abi.fit_req(200, 64)
    refused("16384", req=r)
    for bad in (0.0, 1.0, float("nan")):
        refused("a step must be finite and in (0, 1)", step=np.array([1e-3, bad, 1e-3]))
    refused("out of range", update=False, act=np.array([0, 1, 4], np.int32))
    refused("strictly ascending", update=False, act=np.array([0, 3, 3], np.int32))
    refused("more active elements", update=False, req=abi.fit_req(1, 5), step=np.full(5, 1e-3), act=np.arange(5, dtype=np.int32), g=np.ones((1, 5)))
    refused("n_scalar >= 1", design=False, n_scalar=0)
    refused("more than 65536 scalars", design=False, n_scalar=65537)
    # the design's counts: judged before any array is looked at
    for kinds, text in (((-1, 4, 0), "bad counts (nR, nC, nL >= 0)"), ((4, 0, -2), "bad counts (nR, nC, nL >= 0)"), ((0, 0, 0), "no element (nR + nC + nL = 0)"),
                        ((2 ** 31 - 1, 1, 0), "too many elements"), ((2 ** 30, 0, 0), "too many elements")):   # nE, and n_inst nE, past 2^31 - 1
        with pytest.raises(pf.Refused) as e:
            pf.design(kinds, R, Z, Z, req, act, step, g)
        assert str(e.value).startswith("fit: ") and text in str(e.value), str(e.value)
    with pytest.raises(pf.Refused, match="fit: null buffer"):
        pf.design((4, 0, 0), R, Z, Z, req, None, step, g)
    with pytest.raises(pf.Refused, match="fit: null buffer"):
        pf.update(req, True, step, g_lo, g_hi, None, None, x, g, done)
    for lo, hi in ((0.0, 1.0), (2.0, 1.0), (0.5, float("inf")), (float("nan"), 1.0)):
        refused("0 < g_lo <= g_hi", design=False, g_lo=np.full((1, 3), lo), g_hi=np.full((1, 3), hi))
    for field, bad, text in (("weight", 0.0, "weight"), ("weight", float("inf"), "weight"), ("kind", 4, "unknown goal kind"), ("pad", 1, "pad"), ("lo", float("nan"), "bound"),
                             ("lo", float("inf"), "bound")):
        gl = goals.copy()
        gl[0, 0][field] = bad
        refused(text, design=False, goals=gl)
    gl = goals.copy()
    gl[0, 1] = (abi.FIT_BETWEEN, 0, 2.0, 1.0, 1.0)
    refused("lo <= hi", design=False, goals=gl)
    gl[0, 1] = (abi.FIT_AT_MOST, 0, 0.0, float("inf"), 1.0)
    refused("a goal's bound must be finite", design=False, goals=gl)
    gl[0, 1] = (abi.FIT_BETWEEN, 0, 0.0, float("nan"), 1.0)
    refused("a goal's bound must be finite", design=False, goals=gl)
    L = pf.lib()
    assert L.spicey_fit_host_workspace_bytes(1, 129, 1) == -1 and L.spicey_fit_host_workspace_bytes(1, 1, 0) == -1 and L.spicey_fit_host_workspace_bytes(200, 64, 1) == -1
    assert L.spicey_fit_host_lds_bytes(128) == 132096
