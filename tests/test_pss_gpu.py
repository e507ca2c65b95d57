"""The periodic steady state's kernels on the GPU: spicey_pss_design_device and spicey_pss_update_device on the shapes and the
exact cases of test_pss_host.py, bit for bit against the CPU harness (tests/pss_host) and the numpy restatement; nX = 128 is the
one launch with the full request of dynamic LDS (132 096 bytes).

Bar: bit identity throughout."""
import numpy as np
import pytest

from pss_host import pypss as pp
from spicey_amd import abi
from test_pss_host import _same, check_exact

pytestmark = pytest.mark.gpu


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda() if a is not None and a.size else None


def _ptr(t):
    return t.data_ptr() if t is not None else 0


def _device_design(kinds, req, base, base_on, perturb=True):
    import torch

    from spicey_amd import lib
    base = np.ascontiguousarray(base, dtype=np.float64)
    n_ckt, nX = base.shape
    base_on = np.ascontiguousarray(base_on, dtype=np.int32).reshape(n_ckt, -1)
    nS = base_on.shape[1]
    ni = n_ckt * abi.pss_width(int(req.method), nX)
    d_base, d_on0 = _dev(base), _dev(base_on)
    parts = [torch.full((ni, k), pp.SENTINEL, dtype=torch.float64, device="cuda") if k else None for k in kinds]
    d_on = torch.full((ni, nS), pp.SENTINEL_I, dtype=torch.int32, device="cuda") if nS else None
    d_h = torch.full((n_ckt, nX), pp.SENTINEL, dtype=torch.float64, device="cuda")
    need = lib.pss_workspace_bytes(n_ckt, nX, int(req.method))
    d_work = torch.zeros(need, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    try:
        lib.pss_design_device(kinds, nS, req, _ptr(d_base), _ptr(d_on0), _ptr(d_h), *(_ptr(p) for p in parts), _ptr(d_on), d_work.data_ptr(), need, perturb=perturb)
    finally:
        torch.cuda.synchronize()
    X = np.concatenate([p.cpu().numpy() if p is not None else np.zeros((ni, 0)) for p in parts], axis=1)
    return X, d_on.cpu().numpy() if d_on is not None else np.zeros((ni, 0), np.int32), d_h.cpu().numpy()


def _device_update(kinds, req, base, base_on, h, X, on, done, ist=None):
    import torch

    from spicey_amd import lib
    base = np.ascontiguousarray(base, dtype=np.float64)
    n_ckt, nX = base.shape
    base_on = np.ascontiguousarray(base_on, dtype=np.int32).reshape(n_ckt, -1)
    nS = base_on.shape[1]
    d_base, d_bon, d_h = _dev(base), _dev(base_on), _dev(None if h is None else np.asarray(h, dtype=np.float64))
    parts = [_dev(p) for p in pp.split(np.ascontiguousarray(X, dtype=np.float64), kinds)]
    d_on = _dev(np.ascontiguousarray(on, dtype=np.int32))
    d_done = _dev(np.ascontiguousarray(done, dtype=np.int32))
    d_delta = torch.full((n_ckt, nX), pp.SENTINEL, dtype=torch.float64, device="cuda")
    d_rows = torch.full((n_ckt, abi.PSS_ROW), pp.SENTINEL, dtype=torch.float64, device="cuda")
    need = lib.pss_workspace_bytes(n_ckt, nX, int(req.method))
    d_work = torch.zeros(need, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    try:
        lib.pss_update_device(kinds, nS, req, ist, _ptr(d_base), _ptr(d_bon), _ptr(d_h), *(_ptr(p) for p in parts), _ptr(d_on), d_delta.data_ptr(), d_rows.data_ptr(),
                              d_done.data_ptr(), d_work.data_ptr(), need)
    finally:
        torch.cuda.synchronize()
    return (d_base.cpu().numpy(), d_bon.cpu().numpy() if d_bon is not None else np.zeros((n_ckt, 0), np.int32), d_delta.cpu().numpy(), d_rows.cpu().numpy(),
            d_done.cpu().numpy())


@pytest.mark.parametrize("nX", pp.NX)
def test_design_and_update_device_equal_the_cpu_harness_bit_for_bit(nX):
    for n_ckt in pp.NCKT:
        kinds, req, base, base_on, h, X, on, done, _ = pp.linear_case(nX, n_ckt, seed=100 * nX + n_ckt)
        dX, don, dh = _device_design(kinds, req, base, base_on)
        hX, hon, hh = pp.design(kinds, req, base, base_on)
        assert pp.bits_equal(dX, hX).all() and (don == hon).all() and pp.bits_equal(dh, hh).all(), (nX, n_ckt)
        pX, pon, ph = _device_design(kinds, req, base, base_on, perturb=False)
        assert pp.bits_equal(pX.reshape(n_ckt, 1 + nX, nX), np.broadcast_to(base[:, None, :], (n_ckt, 1 + nX, nX))).all() and (ph == pp.SENTINEL).all()
        got = _device_update(kinds, req, base, base_on, h, X, on, done)
        _same(got, pp.update(kinds, req, base, base_on, h, X, on, done), (nX, n_ckt, "harness"))
        _same(got, pp.reference_update(kinds, req, base, base_on, h, X, on, done), (nX, n_ckt, "numpy"))
        assert (got[3][:, 3] == 1.0).all()


@pytest.mark.parametrize("name", [n for n in pp.EXACT if n != "h_representable"])
def test_exact_small_cases_on_the_device(name):
    k = pp.exact_case(name)
    args = (k["kinds"], k["req"], k["base"], k["base_on"], k["h"], k["X"], k["on"], k["done"], k["ist"])
    got = _device_update(*args)
    _same(got, pp.update(*args), name)
    check_exact(name, k, got)


def test_h_eff_on_the_device_is_the_representable_difference():
    k = pp.exact_case("h_representable")
    X, on, h = _device_design(k["kinds"], k["req"], k["base"], k["base_on"])
    assert pp.bits_equal(h, k["expect"]["h"]).all() and pp.bits_equal(h[0], np.array([X[1, 0], X[2, 1]]) - k["base"][0]).all()


def test_device_refusals_launch_nothing():
    import torch

    from spicey_amd import lib
    from spicey_amd.lib import SpiceyNativeError
    assert lib.pss_workspace_bytes(1, 129, abi.PSS_NEWTON) == -1 and lib.pss_workspace_bytes(1, 0, abi.PSS_SETTLE) == -1
    buf = torch.full((130 * 129,), 7.0, dtype=torch.float64, device="cuda")
    rows = torch.full((8,), 7.0, dtype=torch.float64, device="cuda")
    done = torch.zeros(1, dtype=torch.int32, device="cuda")
    work = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    p = buf.data_ptr()
    for kinds, text in (((129, 0, 0), 'method = "settle"'), ((0, 0, 0), "no state")):
        for call in (lambda: lib.pss_update_device(kinds, 0, abi.pss_req(1), None, p, 0, p, p, 0, 0, 0, 0, rows.data_ptr(), done.data_ptr(), work.data_ptr(), 4096),
                     lambda: lib.pss_design_device(kinds, 0, abi.pss_req(1), p, 0, p, p, 0, 0, 0, work.data_ptr(), 4096)):
            with pytest.raises(SpiceyNativeError) as e:
                call()
            assert e.value.status == abi.ERR_BAD_DESC and "pss: " in str(e.value) and text in str(e.value)
    with pytest.raises(SpiceyNativeError, match="workspace too small"):
        lib.pss_update_device((2, 0, 0), 0, abi.pss_req(1), None, p, 0, p, p, 0, 0, 0, 0, rows.data_ptr(), done.data_ptr(), work.data_ptr(), 8)
    torch.cuda.synchronize()
    assert (buf.cpu().numpy() == 7.0).all() and (rows.cpu().numpy() == 7.0).all() and int(done.cpu()[0]) == 0
