"""Monte Carlo tolerance analysis on the GPU: spicey_ac_mc_draw_device and spicey_ac_mc_reduce_device bit for bit against the CPU
harness (tests/mc_host) and plain numpy, AcHandle.run_mc against a second handle whose rows are the numpy draw's values — its
plain sweep reduced by the harness — on every path a solve can take, the dense fallback included, an invalid sample, a plain
sweep around a Monte Carlo run, and simulateMonteCarlo against the RC closed form.  Every sweep test asserts which kernel ran.

Bars: bit identity for the draw, the reduction and the runs; 3e-9 |ref| + 1e-12 for the closed form (test_mc_host.py)."""
import math

import numpy as np
import pytest

import ac_resident_cases as cases
from mc_host import pymc as pm
from sens_host import pysens as ps
from spicey_amd import abi
from spicey_amd.mc import draw_reference_mc, mc_ranks, mc_values, reduce_reference_mc, simulateMonteCarlo
from spicey_amd.netlist import parseNetlist

pytestmark = pytest.mark.gpu


# (the tests on torch tensors come first: in a process that runs this file alone torch has to open the device before the
# library does, spicey_amd/lib.py load())
def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda() if a.size else None


def _ptr(t):
    return t.data_ptr() if t is not None else 0


def _device_draw(R, Cv, Lv, tol, icdf, req):
    import torch

    from spicey_amd import lib
    ni = R.shape[0]
    d_in = [_dev(a) for a in (R, Cv, Lv)]
    d_out = [torch.full(a.shape, float("nan"), dtype=torch.float64, device="cuda") if a.size else None for a in (R, Cv, Lv)]
    need = lib.ac_mc_workspace_bytes(ni, 1, len(tol), req.log2K, 0)
    d_work = torch.zeros(need, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    try:
        lib.ac_mc_draw_device(ni, R.shape[1], Cv.shape[1], Lv.shape[1], *(_ptr(t) for t in d_in), tol, icdf, req, *(_ptr(t) for t in d_out), d_work.data_ptr(), need)
    finally:
        torch.cuda.synchronize()
    return tuple(t.cpu().numpy() if t is not None else np.zeros(a.shape) for t, a in zip(d_out, (R, Cv, Lv)))


def _device_reduce(d_v, shape, req, valid, lo, hi, ranks):
    import torch

    from spicey_amd import lib
    ni, nf, n_v = shape
    d_sample = torch.full((ni, 2), pm.SENTINEL_I, dtype=torch.int64, device="cuda")
    d_freq = torch.full((nf, abi.MC_FREQ_HEAD + len(ranks)), float("nan"), dtype=torch.float64, device="cuda")
    need = lib.ac_mc_workspace_bytes(ni, nf, 1, 0, len(ranks))
    d_work = torch.zeros(need, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    try:
        lib.ac_mc_reduce_device(ni, nf, d_v.data_ptr(), n_v, valid, lo, hi, ranks, req, d_sample.data_ptr(), d_freq.data_ptr(), d_work.data_ptr(), need)
    finally:
        torch.cuda.synchronize()
    return d_sample.cpu().numpy(), d_freq.cpu().numpy()


@pytest.mark.parametrize("shape", ps.REDUCTION_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_mc_draw_device_equals_the_cpu_harness_and_numpy_bit_for_bit(shape):
    """The draw shapes of test_mc_host.py: nE = 1, 63, 64, 65, 130 with kind borders inside a wave; 1, 2 and 65 samples; tables of
    2, 3 and 1025 entries; keep_first on and off."""
    nE = sum(shape)
    for ni in pm.DRAW_NI:
        for log2K in pm.DRAW_L:
            R, Cv, Lv, tol, icdf = pm.draw_inputs(ni, shape, log2K, seed=100 * nE + 10 * ni + log2K)
            seed = 0x9E3779B97F4A7C15 ^ (nE << 33) ^ ni
            for keep in (False, True):
                req = abi.ac_mc_req(0, -1, log2K, keep, seed)
                got = _device_draw(R, Cv, Lv, tol, icdf, req)
                host = pm.draw(R, Cv, Lv, tol, icdf, req)
                ref = draw_reference_mc(R, Cv, Lv, tol, icdf, log2K, seed, keep)
                for g, h, r, what in zip(got, host, ref, "RCL"):
                    assert g.shape == h.shape and pm.bits_equal(g, h).all() and pm.bits_equal(g, r).all(), (what, shape, ni, log2K, keep)


@pytest.mark.parametrize("ni", pm.REDUCE_NI)
def test_mc_reduce_device_equals_the_cpu_harness_and_numpy_bit_for_bit(ni):
    """The reduction shapes of test_mc_host.py: n_inst around a wave and around the powers of two, 1 to 130 frequencies, the three
    forms of the output pair, the validity masks, a NaN, an inf and equal values among the valid samples, the three masks, ranks at
    0, n_valid - 1 and repeated."""
    for nf in pm.REDUCE_NF:
        v = pm.sweep_like(ni, nf, 3, seed=1000 * ni + nf)
        d_v = _dev(v)
        for j, (op, on) in enumerate(pm.PAIRS):
            req = abi.ac_mc_req(op, on, 0, False, 0)
            for kind in pm.VALIDITY:
                valid = pm.validity(kind, ni)
                n_valid = ni if valid is None else int(valid.sum())
                if n_valid == 0:
                    continue
                ranks = pm.rank_cases(n_valid)
                for mk in pm.MASKS:
                    lo, hi = pm.limits(mk, nf, seed=j)
                    sample, freq = _device_reduce(d_v, v.shape, req, valid, lo, hi, ranks)
                    hs, hf = pm.reduce(v, req, valid, lo, hi, ranks)
                    rs, rf = reduce_reference_mc(v, op, on, valid, lo, hi, ranks)
                    assert (sample == hs).all() and (sample == rs).all(), (ni, nf, op, on, kind, mk)
                    assert pm.bits_equal(freq, hf).all() and pm.bits_equal(freq, rf).all(), (ni, nf, op, on, kind, mk)


@pytest.mark.parametrize("ni", (16384, 8193))
def test_mc_reduce_device_at_the_largest_sort(ni):
    """n_pad = 16384: 128 KiB of keys in LDS, 1024 threads, 105 stages; 8193 samples pad the upper half."""
    nf = 2
    v = pm.sweep_like(ni, nf, 2, seed=ni)
    valid = pm.validity("third", ni)
    ranks = mc_ranks((0.0, 0.01, 0.5, 0.99, 1.0), int(valid.sum()))
    lo, hi = pm.limits("both", nf)
    req = abi.ac_mc_req(0, 1, 0, False, 0)
    sample, freq = _device_reduce(_dev(v), v.shape, req, valid, lo, hi, ranks)
    hs, hf = pm.reduce(v, req, valid, lo, hi, ranks)
    rs, rf = reduce_reference_mc(v, 0, 1, valid, lo, hi, ranks)
    assert (sample == hs).all() and (sample == rs).all()
    assert pm.bits_equal(freq, hf).all() and pm.bits_equal(freq, rf).all()


def test_mc_device_refusals_launch_nothing():
    import torch

    from spicey_amd import lib
    from spicey_amd.lib import SpiceyNativeError
    shape = (4, 2, 1)
    R, Cv, Lv, tol, icdf = pm.draw_inputs(3, shape, 3, seed=7)
    d_in = [_dev(a) for a in (R, Cv, Lv)]
    outs = [torch.full(a.shape, 7.0, dtype=torch.float64, device="cuda") for a in (R, Cv, Lv)]
    need = lib.ac_mc_workspace_bytes(3, 4, 7, 3, 2)
    d_work = torch.zeros(need, dtype=torch.uint8, device="cuda")
    ok = abi.ac_mc_req(0, -1, 3, True, 5)

    def req(**kw):
        q = abi.ac_mc_req(0, -1, 3, True, 5)
        for k, val in kw.items():
            setattr(q, k, val)
        return q
    neg, nan, big, dec, inf = tol.copy(), tol.copy(), tol.copy(), icdf.copy(), icdf.copy()
    neg[3], nan[6], big[0], dec[4], inf[8] = -0.01, np.nan, 1.0 / np.abs(icdf).max(), icdf[3] - 1e-9, np.inf
    for q, ni, tl, tab, wb in ((req(struct_bytes=8), 3, tol, icdf, need), (req(reserved=1), 3, tol, icdf, need), (req(log2K=13), 3, tol, icdf, need),
                               (ok, 0, tol, icdf, need), (ok, 16385, tol, icdf, need), (ok, 3, neg, icdf, need), (ok, 3, nan, icdf, need), (ok, 3, big, icdf, need),
                               (ok, 3, tol, dec, need), (ok, 3, tol, inf, need), (ok, 3, None, icdf, need), (ok, 3, tol, None, need), (ok, 3, tol, icdf, 8),
                               (None, 3, tol, icdf, need)):
        with pytest.raises(SpiceyNativeError) as e:
            lib.ac_mc_draw_device(ni, 4, 2, 1, *(t.data_ptr() for t in d_in), tl, tab, q, *(t.data_ptr() for t in outs), d_work.data_ptr(), wb)
        assert e.value.status == abi.ERR_BAD_DESC and "mc" in str(e.value)
    with pytest.raises(SpiceyNativeError, match="no element"):
        lib.ac_mc_draw_device(3, 0, 0, 0, 0, 0, 0, tol, icdf, ok, 0, 0, 0, d_work.data_ptr(), need)
    with pytest.raises(SpiceyNativeError, match="null buffer"):
        lib.ac_mc_draw_device(3, 4, 2, 1, *(t.data_ptr() for t in d_in), tol, icdf, ok, outs[0].data_ptr(), 0, outs[2].data_ptr(), d_work.data_ptr(), need)
    # the reduction
    v = pm.sweep_like(3, 4, 3, seed=11, plant=False)
    d_v = _dev(v)
    d_sample = torch.full((3, 2), 7, dtype=torch.int64, device="cuda")
    d_freq = torch.full((4, 6), 7.0, dtype=torch.float64, device="cuda")
    ranks = np.array([0, 2], np.int64)
    one_bad = np.array([1, 0, 1], np.uint8)
    rok = abi.ac_mc_req(0, -1, 0, False, 0)
    for q, ni, nf, n_v, valid, rk, wb in ((abi.ac_mc_req(3, -1, 0, False, 0), 3, 4, 3, None, ranks, need), (abi.ac_mc_req(1, 1, 0, False, 0), 3, 4, 3, None, ranks, need),
                                          (abi.ac_mc_req(-1, -1, 0, False, 0), 3, 4, 3, None, ranks, need), (req(struct_bytes=48), 3, 4, 3, None, ranks, need),
                                          (rok, 0, 4, 3, None, ranks, need), (rok, 3, 0, 3, None, ranks, need), (rok, 3, 4, 0, None, ranks, need),
                                          (rok, 16385, 4, 3, None, ranks, need), (rok, 3, 4, 3, None, np.array([0, 3], np.int64), need),
                                          (rok, 3, 4, 3, one_bad, ranks, need), (rok, 3, 4, 3, None, np.array([-1, 0], np.int64), need), (rok, 3, 4, 3, None, ranks, 8),
                                          (None, 3, 4, 3, None, ranks, need)):
        with pytest.raises(SpiceyNativeError) as e:
            lib.ac_mc_reduce_device(ni, nf, d_v.data_ptr(), n_v, valid, None, None, rk, q, d_sample.data_ptr(), d_freq.data_ptr(), d_work.data_ptr(), wb)
        assert e.value.status == abi.ERR_BAD_DESC and "mc" in str(e.value)
    with pytest.raises(SpiceyNativeError, match="null buffer"):
        lib.ac_mc_reduce_device(3, 4, d_v.data_ptr(), 3, None, None, None, ranks, rok, 0, d_freq.data_ptr(), d_work.data_ptr(), need)
    with pytest.raises(SpiceyNativeError, match="null buffer"):
        lib.ac_mc_reduce_device(3, 4, 0, 3, None, None, None, ranks, rok, d_sample.data_ptr(), d_freq.data_ptr(), d_work.data_ptr(), need)
    torch.cuda.synchronize()
    assert all((o.cpu().numpy() == 7.0).all() for o in outs) and (d_work.cpu().numpy() == 0).all()
    assert (d_sample.cpu().numpy() == 7).all() and (d_freq.cpu().numpy() == 7.0).all()
    W = lib.ac_mc_workspace_bytes
    assert W(0, 4, 7, 3, 2) == -1 and W(16385, 4, 7, 3, 2) == -1 and W(3, 4, 7, 13, 2) == -1 and W(3, 4, 0, 3, 2) == -1 and W(3, 0, 7, 3, 2) == -1


# ---- a run on a handle ---------------------------------------------------------------------------------------------------
PROBS = (0.0, 0.01, 0.5, 0.99, 1.0)


def _mc_tol(flat, r=0.02, c=0.05, ind=0.03):
    """Per-element tolerances with zeros among them."""
    t = np.concatenate([np.full(flat.nR, r), np.full(flat.nC, c), np.full(flat.nL, ind)])
    t[::7] = 0.0
    return t


def _run_mc_against_a_handle_of_the_drawn_values(flat, freqs, vph, req, tol, icdf, kw, mode, lo=None, hi=None, expect=(abi.OK,)):
    """AcHandle.run_mc on `flat`, and a second handle created from the FlatCircuit whose rows are the numpy draw's values: its
    plain run reduced by the harness gives the same bits.  A plain run before and after run_mc gives identical bits."""
    from spicey_amd.lib import AcHandle
    h = AcHandle(flat, **kw)
    before = h.run(freqs, vph, want_currents=False)
    res = h.run_mc(freqs, vph, req, tol, icdf, lo, hi, PROBS)
    info = h.info()
    assert res["status"] in expect and info["interpreter"] == mode, (res["detail"], info)
    after = h.run(freqs, vph, want_currents=False)
    h.close()
    assert before["status"] == after["status"] and pm.bits_equal(before["out_v"].view(np.float64), after["out_v"].view(np.float64)).all()

    def second(f, fr, ph):
        h2 = AcHandle(f, **kw)
        r = h2.run(fr, ph, want_currents=False)
        assert h2.info()["interpreter"] == mode
        h2.close()
        return r
    ref = pm.run_mc_reference(second, flat, freqs, vph, req, tol, icdf, lo, hi, PROBS)
    assert res["status"] == ref["status"] and (res["inst_status"] == ref["inst_status"]).all()
    assert (res["sample"] == ref["sample"]).all()
    assert res["freq_stats"].shape == ref["freq_stats"].shape and pm.bits_equal(res["freq_stats"], ref["freq_stats"]).all()
    if req.keep_first:
        assert pm.bits_equal(res["nominal"].view(np.float64), ref["nominal"].view(np.float64)).all()
        assert pm.bits_equal(res["nominal"].view(np.float64), (before["out_v"][0, :, req.out_p] - (before["out_v"][0, :, req.out_n] if req.out_n >= 0 else 0)).view(np.float64)).all()
    # the drawn values did reach the sweep: the band is open
    fs = res["freq_stats"]
    assert (fs[:, 4] < fs[:, 4 + 2 * len(PROBS) - 1]).any()
    assert res["mc_ms"] > 0 and res["draw_ms"] > 0 and res["kernel_ms"] > 0
    return res, info, ref


PATHS = ((dict(threads=64), 2), (dict(no_resident=True), 1), (dict(force_global=True), 1), (dict(interpreter=3), 3))
PATH_IDS = ("resident", "per_solve", "global", "exact_order")


@pytest.mark.parametrize("kw,mode", PATHS, ids=PATH_IDS)
def test_run_mc_on_a_fed_ladder_equals_a_handle_of_the_drawn_values(kw, mode):
    """fed_ladder(68, 47), 34 samples x 16 frequencies (544 slots: just enough for the resident kernel) with nominal rows and
    phasors of their own, the pair (c30, c4), a Gaussian table, a mask with both sides."""
    flat, freqs, vph = cases.fed_ladder_case()
    flat.out_nodes = np.array([4, 30], np.int32)
    from spicey_amd.mc import icdf_table
    icdf, log2K = icdf_table("gauss")
    req = abi.ac_mc_req(1, 0, log2K, True, 2024)
    lo, hi = np.full(len(freqs), 1e-3), np.full(len(freqs), 0.5)
    res, info, _ = _run_mc_against_a_handle_of_the_drawn_values(flat, freqs, vph, req, _mc_tol(flat), icdf, kw, mode, lo, hi)
    assert np.isfinite(res["freq_stats"]).all() and (res["freq_stats"][:, 0] == flat.n_inst).all()
    if mode == 1:
        assert (info["lds_bytes"] == 0) == ("force_global" in kw)


@pytest.mark.parametrize("kw,mode", PATHS, ids=PATH_IDS)
def test_run_mc_on_a_mesh_equals_a_handle_of_the_drawn_values(kw, mode):
    """rlc6x6, 34 samples x 16 frequencies, one node against ground, a uniform table, no mask, sample 0 drawn too."""
    flat, freqs, vph = cases.mesh_case("rlc6x6")
    flat.out_nodes = np.array([flat.n_nodes], np.int32)
    req = abi.ac_mc_req(0, -1, 0, False, 7)
    res, _, _ = _run_mc_against_a_handle_of_the_drawn_values(flat, freqs, vph, req, _mc_tol(flat), np.array([-1.0, 1.0]), kw, mode)
    assert res["nominal"] is None and (res["sample"] == [0, -1]).all()


def test_run_mc_reaches_the_dense_fallback():
    """ladder_case at its resonant frequencies, 64 samples: the resistors are drawn, L and C stay nominal, so the near-resonant
    slots still trip the static pivot order and are repeated dense — with the drawn 1 / R."""
    flat, freqs, vph, near = cases.ladder_case(64)
    flat.out_nodes = np.array([3], np.int32)  # (node b0, between L0 and C0)
    tol = np.concatenate([np.full(flat.nR, 0.05), np.zeros(flat.nC + flat.nL)])
    req = abi.ac_mc_req(0, -1, 0, True, 99)
    res, info, ref = _run_mc_against_a_handle_of_the_drawn_values(flat, freqs, vph, req, tol, np.array([-1.0, 1.0]), {}, 2)
    assert near.any(axis=1).sum() <= info["tail_levels"] <= near.sum() and info["tail_levels"] > 0, info
    assert np.isfinite(res["freq_stats"]).all()
    # at a resonance |H| is Q-multiplied, so the drawn resistances show there: the fallback did read them
    k = int(np.argmax(near.any(axis=0)))
    assert res["freq_stats"][k, 4] < res["freq_stats"][k, 4 + 2 * len(PROBS) - 1]


def test_run_mc_leaves_an_invalid_sample_out():
    """sing_case, 40 samples of which number 17 is singular at its first frequency, zero tolerances: n_valid = n_inst - 1, the bad
    sample's row is {-1, -1}, and the statistics are those of the other samples' plain sweep."""
    from spicey_amd.lib import AcHandle
    flat, freqs, vph, keep_flat, keep_vph = cases.sing_case(40, 17)
    n_out = flat.n_nodes
    tol = np.zeros(flat.nR + flat.nC + flat.nL)
    req = abi.ac_mc_req(n_out - 1, -1, 0, True, 1)
    lo = np.full(len(freqs), 0.0)
    h = AcHandle(flat)
    res = h.run_mc(freqs, vph, req, tol, np.array([-1.0, 1.0]), lo, None, PROBS)
    h.close()
    assert res["status"] == abi.ERR_SINGULAR and res["inst_status"][17] == abi.ERR_SINGULAR and np.count_nonzero(res["inst_status"]) == 1
    assert (res["freq_stats"][:, 0] == 39).all() and (res["sample"][17] == -1).all() and (np.delete(res["sample"], 17, axis=0)[:, 0] >= 0).all()
    h2 = AcHandle(keep_flat)
    plain = h2.run(freqs, keep_vph, want_currents=False)
    h2.close()
    assert plain["status"] == abi.OK
    sample, freq = pm.reduce(plain["out_v"], req, None, lo, None, mc_ranks(PROBS, 39))
    assert pm.bits_equal(res["freq_stats"], freq).all() and (np.delete(res["sample"], 17, axis=0) == sample).all()


def test_run_mc_refusals_run_nothing():
    from spicey_amd.lib import AcHandle
    flat, freqs, vph = cases.fed_ladder_case(4)
    flat.out_nodes = np.array([4, 30], np.int32)
    tol = _mc_tol(flat)
    uni = np.array([-1.0, 1.0])
    h = AcHandle(flat)
    ok = abi.ac_mc_req(1, 0, 0, True, 3)
    bad_tol, nan_tab = tol.copy(), uni.copy()
    bad_tol[1], nan_tab[1] = -0.1, np.nan
    cases_ = ((abi.ac_mc_req(2, 0, 0, True, 3), tol, uni, PROBS), (abi.ac_mc_req(0, 0, 0, True, 3), tol, uni, PROBS), (ok, bad_tol, uni, PROBS),
              (ok, np.ones_like(tol), uni, PROBS), (ok, tol, nan_tab, PROBS), (ok, tol, uni, (0.5, 1.5)), (ok, tol, uni, (math.nan,)))
    for q, tl, tab, pr in cases_:
        res = h.run_mc(freqs, vph, q, tl, tab, None, None, pr)
        assert res["status"] == abi.ERR_BAD_DESC and "mc" in res["detail"], res["detail"]
        assert (res["freq_stats"] == 0).all() and (res["sample"] == 0).all() and res["mc_ms"] == 0 and res["draw_ms"] == 0
    q = abi.ac_mc_req(1, 0, 0, True, 3)
    q.reserved = 1
    assert h.run_mc(freqs, vph, q, tol, uni)["status"] == abi.ERR_BAD_DESC
    assert h.run_mc(freqs, vph, ok, tol, uni, probs=PROBS)["status"] == abi.OK
    h.close()


# ---- the public interface ---------------------------------------------------------------------------------------------------
RC = "V1 in 0 AC 1\nR1 in out 1000\nC1 out 0 1e-9\n.ac dec 5 1e3 1e7\n.end\n"


def test_simulate_monte_carlo_rc_against_the_closed_form_and_the_numpy_count():
    ckt = parseNetlist(RC)
    tol, n, seed, probs = {"R1": 0.01, "C": 0.05}, 200, 5, (0.01, 0.5, 0.99)
    mask = [(1.2e5, 2.0e5, 0.70, None)]
    r = simulateMonteCarlo(ckt, "v(out)", tol=tol, n=n, seed=seed, quantiles=probs, mask=mask)
    f = np.array(r["freq"])
    q, curves = pm.rc_closed_form(ckt, tol, seed, n, f, probs)
    assert r["n_valid"] == n
    for p, ref in zip(probs, curves):
        got = np.array(r["mag"][p])
        assert (np.abs(got - ref) <= 3e-9 * np.abs(ref) + 1e-12).all(), (p, np.abs(got - ref).max())
    h = 1 / (1 + 2j * np.pi * f * 1e-6)
    assert (np.abs(np.array(r["nominal"]) - h) <= 3e-9 * np.abs(h) + 1e-12).all()
    sel = (f >= 1.2e5) & (f <= 2.0e5)
    viol = np.zeros_like(q, bool)
    viol[:, sel] = q[:, sel] < 0.70 * 0.70
    assert sel.sum() == 1 and 0 < viol.any(axis=1).sum() < n
    assert r["viol_per_freq"] == viol.sum(axis=0).tolist() and r["yield"] == 1.0 - viol.any(axis=1).sum() / n
    assert r["failing"] == [(int(s), int(viol[s].sum()), float(f[int(np.argmax(viol[s]))])) for s in np.nonzero(viol.any(axis=1))[0]]
    s = r["failing"][0][0]
    vals = mc_values(ckt, tol, seed, s)
    assert 1.0 / (1.0 + (2 * math.pi * r["failing"][0][2] * vals["R1"] * vals["C1"]) ** 2) < 0.49
    # the reference-order engine runs the same analysis
    x = simulateMonteCarlo(ckt, "v(out)", tol=tol, n=n, seed=seed, quantiles=probs, mask=mask, exact_order=True)
    assert x["yield"] == r["yield"] and np.allclose(x["mag"][0.5], r["mag"][0.5], rtol=3e-9)
