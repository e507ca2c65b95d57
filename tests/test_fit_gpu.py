"""The element sizing's kernels on the GPU: spicey_fit_design_device and spicey_fit_update_device on the shapes and the exact
cases of test_fit_host.py, bit for bit against the CPU harness (tests/fit_host) and the numpy restatement — the gains, the rows,
done and the circuits' state in the workspace; nA = 128 is the one launch with the full request of dynamic LDS (132 096 bytes).
Outputs start as sentinels, so what a kernel did not write shows; the refusals launch nothing.

Bar: bit identity throughout."""
import numpy as np
import pytest

from fit_host import pyfit as pf
from spicey_amd import abi, fit
from test_fit_host import _same, check_exact, reference_exact, run_exact

pytestmark = pytest.mark.gpu


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda() if a is not None and a.size else None


def _ptr(t):
    return t.data_ptr() if t is not None else 0


def _device_design(kinds, R, Cv, Lv, req, act, step, g):
    import torch

    from spicey_amd import lib
    ins = [_dev(np.asarray(a, dtype=np.float64)) for a in (R, Cv, Lv)]
    outs = [torch.full(a.shape, pf.SENTINEL, dtype=torch.float64, device="cuda") if a.size else None for a in (R, Cv, Lv)]
    d_g = _dev(np.asarray(g, dtype=np.float64))
    need = lib.fit_workspace_bytes(int(req.n_ckt), int(req.nA), 1)
    d_work = torch.zeros(need, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    try:
        lib.fit_design_device(*kinds, *(_ptr(t) for t in ins), req, act, step, _ptr(d_g), *(_ptr(t) for t in outs), d_work.data_ptr(), need)
    finally:
        torch.cuda.synchronize()
    return tuple(o.cpu().numpy() if o is not None else np.zeros(a.shape) for o, a in zip(outs, (R, Cv, Lv)))


def _device_update(req, first, step, g_lo, g_hi, goals, valid, x, g, done, work=None, rows=None, **_):
    """pf.update's signature on the device; work: a torch uint8 tensor that carries the state (None: a fresh one)."""
    import torch

    from spicey_amd import lib
    g = np.ascontiguousarray(g, dtype=np.float64)
    n_ckt, nA = g.shape
    x = np.ascontiguousarray(x, dtype=np.float64)
    ns = x.shape[-1]
    need = lib.fit_workspace_bytes(n_ckt, nA, ns)
    if work is None:
        work = torch.zeros(need, dtype=torch.uint8, device="cuda")
    d_x, d_g, d_done = _dev(x), _dev(g), _dev(np.ascontiguousarray(done, dtype=np.int32))
    d_rows = _dev(np.full((n_ckt, abi.FIT_ROW), pf.SENTINEL) if rows is None else np.asarray(rows, dtype=np.float64))
    torch.cuda.synchronize()
    try:
        lib.fit_update_device(req, ns, first, step, g_lo, g_hi, goals, valid, d_x.data_ptr(), d_g.data_ptr(), d_rows.data_ptr(), d_done.data_ptr(), work.data_ptr(), need)
    finally:
        torch.cuda.synchronize()
    return d_g.cpu().numpy(), d_rows.cpu().numpy(), d_done.cpu().numpy(), pf.state_of(work.cpu().numpy(), n_ckt, nA, ns)


def _new_work(n_ckt, nA, ns):
    import torch

    from spicey_amd import lib
    return torch.zeros(lib.fit_workspace_bytes(n_ckt, nA, ns), dtype=torch.uint8, device="cuda")


_device_update.new_work = _new_work


@pytest.mark.parametrize("nA", pf.NA)
def test_design_device_equals_the_cpu_harness_bit_for_bit(nA):
    for n_ckt in pf.NCKT:
        rng = np.random.default_rng(10 * nA + n_ckt)
        ni = n_ckt * (1 + 2 * nA)
        kinds = ((nA + 2) // 3 + 1, (nA + 1) // 3 + 1, nA // 3 + 2)
        R, Cv, Lv = (rng.uniform(0.5, 2.0, (ni, k)) * 10.0 ** rng.integers(-9, 4) for k in kinds)
        act = np.sort(rng.choice(sum(kinds), nA, replace=False)).astype(np.int32)
        step = rng.choice([1e-3, 2.0 ** -9, 5e-4], nA)
        g = rng.uniform(0.3, 3.0, (n_ckt, nA))
        req = abi.fit_req(n_ckt, nA)
        got = _device_design(kinds, R, Cv, Lv, req, act, step, g)
        for a, b, c in zip(got, pf.design(kinds, R, Cv, Lv, req, act, step, g), fit.design_reference_fit(R, Cv, Lv, act, step, g)):
            assert pf.bits_equal(a, b).all() and pf.bits_equal(a, c).all(), (nA, n_ckt)
    # a kind that is absent: its arrays are null
    R = np.array([[2.0, 3.0]] * 3)
    got = _device_design((2, 0, 0), R, np.zeros((3, 0)), np.zeros((3, 0)), abi.fit_req(1, 1), np.array([1], np.int32), np.array([0.5]), np.array([[2.0]]))
    assert got[0].tolist() == [[2.0, 6.0], [2.0, 9.0], [2.0, 3.0]]


@pytest.mark.parametrize("n_scalar", pf.NSCALAR)
@pytest.mark.parametrize("nA", pf.NA)
def test_update_device_equals_the_cpu_harness_bit_for_bit(nA, n_scalar):
    """test_fit_host.py's two updates on one workspace: an accepted first point, then an accepted point, one with a frozen column
    and a rejected one beside it."""
    for n_ckt in pf.NCKT:
        req, step, g_lo, g_hi, goals, x, g, done = pf.random_case(nA, n_scalar, n_ckt, seed=1000 * nA + 10 * n_scalar + n_ckt)
        d_work, work = _new_work(n_ckt, nA, n_scalar), pf.workspace(n_ckt, nA, n_scalar)
        got = _device_update(req, True, step, g_lo, g_hi, goals, None, x, g, done, d_work)
        host = pf.update(req, True, step, g_lo, g_hi, goals, None, x, g, done, work)
        _same(got, host, (nA, n_scalar, n_ckt, "harness"))
        _same(got, pf.reference_update(req, True, step, g_lo, g_hi, goals, None, x, g, done), (nA, n_scalar, n_ckt, "numpy"))
        assert (got[1][:, 4] == 1.0).all()
        x2 = x.copy()
        W = 1 + 2 * nA
        valid = None
        for c in range(min(n_ckt, 2)):
            x2[c * W:(c + 1) * W, 0] = 0.5 * (x[c * W:(c + 1) * W, 0] + goals[c, 0]["lo"])
        if n_ckt > 1:
            x2[W + 1, 0] = np.nan
            valid = np.ones(n_ckt * W, np.uint8)
            valid[2 * W + 2 * nA] = 0
        got2 = _device_update(req, False, step, g_lo, g_hi, goals, valid, x2, got[0], got[2], d_work, rows=got[1])
        _same(got2, pf.update(req, False, step, g_lo, g_hi, goals, valid, x2, host[0], host[2], work, rows=host[1]), (nA, n_scalar, n_ckt, "second"))
        assert got2[1][0, 3] == 1.0 and (n_ckt == 1 or (got2[1][1, 6] == 1.0 and got2[1][2, 3] == 0.0))


@pytest.mark.parametrize("name", pf.EXACT)
def test_exact_small_cases_on_the_device(name):
    k, out = run_exact(name, _device_update)
    for n, (got, ref) in enumerate(zip(out, reference_exact(k))):
        _same(got, ref, (name, n))
    for n, (got, host) in enumerate(zip(out, run_exact(name)[1])):
        _same(got, host, (name, n, "harness"))
    check_exact(name, k, out)


def test_device_refusals_launch_nothing():
    import torch

    from spicey_amd import lib
    from spicey_amd.lib import SpiceyNativeError
    assert lib.fit_workspace_bytes(1, 129, 1) == -1 and lib.fit_workspace_bytes(1, 1, 0) == -1 and lib.fit_workspace_bytes(200, 64, 1) == -1
    buf = torch.full((64,), 7.0, dtype=torch.float64, device="cuda")
    rows = torch.full((8,), 7.0, dtype=torch.float64, device="cuda")
    done = torch.zeros(1, dtype=torch.int32, device="cuda")
    work = torch.zeros(1 << 16, dtype=torch.uint8, device="cuda")
    p = buf.data_ptr()
    goal = abi.fit_goals([(abi.FIT_EQ, 1.0, 1.0, 1.0)])
    one = np.array([0.5])

    def update(req=abi.fit_req(1, 1), step=one, lo=one, hi=one, goals=goal, ns=1, wb=1 << 16):
        lib.fit_update_device(req, ns, True, step, lo, hi, goals, None, p, p, rows.data_ptr(), done.data_ptr(), work.data_ptr(), wb)

    def design(req=abi.fit_req(1, 1), act=np.array([0], np.int32), step=one, wb=1 << 16):
        lib.fit_design_device(1, 0, 0, p, 0, 0, req, act, step, p, p, 0, 0, work.data_ptr(), wb)

    bad_req = abi.fit_req(1, 1)
    bad_req.lam_up = 1.0
    big = abi.fit_req(1, 129)
    for call, text in ((lambda: update(req=big), "128"), (lambda: design(req=big), "128"), (lambda: update(req=bad_req), "lam_up"), (lambda: update(wb=8), "workspace too small"),
                       (lambda: design(wb=8), "workspace too small"), (lambda: update(ns=0), "n_scalar"), (lambda: update(step=np.array([1.0])), "a step"),
                       (lambda: update(lo=np.array([0.0])), "g_lo"), (lambda: update(goals=abi.fit_goals([(abi.FIT_EQ, 1.0, 1.0, 0.0)])), "weight"),
                       (lambda: design(act=np.array([1], np.int32)), "out of range"), (lambda: update(req=None), "null request")):
        with pytest.raises(SpiceyNativeError) as e:
            call()
        assert e.value.status == abi.ERR_BAD_DESC and "fit: " in str(e.value) and text in str(e.value), str(e.value)
    torch.cuda.synchronize()
    assert (buf.cpu().numpy() == 7.0).all() and (rows.cpu().numpy() == 7.0).all() and int(done.cpu()[0]) == 0 and int(work.cpu().max()) == 0
