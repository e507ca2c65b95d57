"""AC sensitivity analysis on the GPU: spicey_ac_sens_device bit for bit against the CPU harness (tests/sens_host) and plain
numpy, AcHandle.run_sens against the harness reduction of the same handle's own plain and injected sweeps on every path a solve
can take, simulateSensBatch against single calls, the RC closed form through the public API, and a plain sweep around a sens
run.  Every sweep test asserts which kernel ran.

Bars: bit identity for the reduction; 3e-9 |ref| + 1e-12 for the closed form (test_sens_host.py)."""
import numpy as np
import pytest

import ac_resident_cases as cases
from batch_variants import variant
from sens_host import pysens as ps
from spicey_amd import abi
from spicey_amd.netlist import parseNetlist
from spicey_amd.sens import reduce_reference_sens, simulateSens, simulateSensBatch

pytestmark = pytest.mark.gpu


# (the tests on torch tensors come first: in a process that runs this file alone torch has to open the device before the
# library does, spicey_amd/lib.py load())
def _device_sens(out_v, i_dir, i_adj, R, Cv, Lv, tol, freqs, req, full):
    """spicey_ac_sens_device on torch tensors; (spec, peak, full or None) back on the host."""
    import torch

    from spicey_amd import lib
    ni, nf, n_v = out_v.shape
    nE = len(tol)

    def dev(a):
        return torch.from_numpy(np.ascontiguousarray(a)).cuda() if a.size else None
    d_v, d_id, d_ix, d_R, d_C, d_L, d_f = (dev(a) for a in (out_v, i_dir, i_adj, R, Cv, Lv, freqs))
    nan = float("nan")
    d_spec = torch.full((ni, nf, abi.SENS_SPEC), nan, dtype=torch.float64, device="cuda")
    d_peak = torch.full((ni, nE, abi.SENS_PEAK), nan, dtype=torch.float64, device="cuda")
    d_full = torch.full((ni, nf, nE, 2), nan, dtype=torch.float64, device="cuda") if full else None
    need = lib.ac_sens_workspace_bytes(ni, nf, nE)
    d_work = torch.zeros(max(need, 8), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    try:
        lib.ac_sens_device(ni, nf, d_v.data_ptr(), n_v, d_id.data_ptr(), d_ix.data_ptr(), i_dir.shape[2], *(t.data_ptr() if t is not None else 0 for t in (d_R, d_C, d_L)),
                           tol, d_f.data_ptr(), req, d_spec.data_ptr(), d_peak.data_ptr(), d_full.data_ptr() if full else 0, d_work.data_ptr(), need)
    finally:
        torch.cuda.synchronize()
    return d_spec.cpu().numpy(), d_peak.cpu().numpy(), d_full.cpu().numpy() if full else None


@pytest.mark.parametrize("shape", ps.REDUCTION_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_sens_device_equals_the_cpu_harness_and_numpy_bit_for_bit(shape):
    """The reduction shapes of test_sens_host.py: nE = 1, 63, 64, 65, 130 with kind borders inside a wave, one, two and 17
    frequencies, three instances, the three windows, the three forms of the output pair, the first frequency 0, H = 0 in one
    slot, tolerances with zeros; with d_full and without, d_peak and d_spec the same both ways."""
    nR, nC, nL = shape
    nE = nR + nC + nL
    for nf in ps.REDUCTION_NF:
        out_v, i_dir, i_adj, R, Cv, Lv, tol, freqs = ps.sens_inputs(3, nf, shape, 3, 3, seed=1000 * nE + nf)
        freqs[0] = 0.0
        out_v[1, nf // 2, :] = 0.0
        for (k0, k1) in ps.windows(nf):
            for (op, on) in ps.REDUCTION_PAIRS:
                req = abi.ac_sens_req(op, on, nR, nC, nL, k0, k1)
                got = _device_sens(out_v, i_dir, i_adj, R, Cv, Lv, tol, freqs, req, True)
                lean = _device_sens(out_v, i_dir, i_adj, R, Cv, Lv, tol, freqs, req, False)
                with np.errstate(all="ignore"):
                    host = ps.reduce(out_v, i_dir, i_adj, R, Cv, Lv, tol, freqs, req, full=True)
                ref = reduce_reference_sens(out_v, i_dir, i_adj, R, Cv, Lv, tol, freqs, op, on, k0, k1)
                for g, h, r, what in zip(got, host, ref, ("spec", "peak", "full")):
                    assert ps.bits_equal(g, h).all() and ps.bits_equal(g, r).all(), (what, shape, nf, k0, k1, op, on)
                assert lean[2] is None and ps.bits_equal(lean[0], got[0]).all() and ps.bits_equal(lean[1], got[1]).all()


def test_sens_device_refusal_launches_nothing():
    import torch

    from spicey_amd import lib
    from spicey_amd.lib import SpiceyNativeError
    shape = (4, 2, 1)
    out_v, i_dir, i_adj, R, Cv, Lv, tol, freqs = ps.sens_inputs(2, 5, shape, 2, 2, seed=7)
    d = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (out_v, i_dir, i_adj, R, Cv, Lv, freqs)]
    outs = [torch.full(s, 7.0, dtype=torch.float64, device="cuda") for s in ((2, 5, 6), (2, 7, 4), (2, 5, 7, 2))]
    need = lib.ac_sens_workspace_bytes(2, 5, 7)
    d_work = torch.zeros(need, dtype=torch.uint8, device="cuda")
    bad_tol = tol.copy()
    bad_tol[3] = -0.01
    nan_tol = tol.copy()
    nan_tol[6] = np.nan
    ok = (0, -1, 4, 2, 1)
    for req, tl, wb in ((abi.ac_sens_req(2, -1, 4, 2, 1), tol, need), (abi.ac_sens_req(0, 0, 4, 2, 1), tol, need), (abi.ac_sens_req(*ok, 3, 2), tol, need),
                        (abi.ac_sens_req(*ok), tol, need - 8), (abi.ac_sens_req(*ok), bad_tol, need), (abi.ac_sens_req(*ok), nan_tol, need),
                        (abi.ac_sens_req(*ok), None, need), (abi.ac_sens_req(0, -1, 4, 2, 4), tol, need), (abi.ac_sens_req(0, -1, 0, 0, 0), tol, need)):
        with pytest.raises(SpiceyNativeError) as e:
            lib.ac_sens_device(2, 5, d[0].data_ptr(), 2, d[1].data_ptr(), d[2].data_ptr(), 9, d[3].data_ptr(), d[4].data_ptr(), d[5].data_ptr(), tl, d[6].data_ptr(),
                               req, outs[0].data_ptr(), outs[1].data_ptr(), outs[2].data_ptr(), d_work.data_ptr(), wb)
        assert e.value.status == abi.ERR_BAD_DESC and "sens" in str(e.value)
    torch.cuda.synchronize()
    assert all((o.cpu().numpy() == 7.0).all() for o in outs) and (d_work.cpu().numpy() == 0).all()
    assert lib.ac_sens_workspace_bytes(0, 5, 7) == -1 and lib.ac_sens_workspace_bytes(2, 5, 0) == -1


def _run_sens_against_its_own_sweeps(flat, freqs, vph, node_p, node_n, req, tol, kw, mode):
    """AcHandle.run_sens, then run and run_inject on the same handle reduced by the harness: the same bits."""
    from spicey_amd.lib import AcHandle
    h = AcHandle(flat, **kw)
    res = h.run_sens(freqs, vph, node_p, node_n, req, tol, full=True)
    info = h.info()
    assert res["status"] == 0 and info["interpreter"] == mode, (res["detail"], info)
    d = h.run(freqs, vph)
    assert d["status"] == 0 and h.info()["interpreter"] == mode
    x = h.run_inject(freqs, None, node_p, node_n)
    assert x["status"] == 0 and h.info()["interpreter"] == mode
    lean = h.run_sens(freqs, vph, node_p, node_n, req, tol)
    h.close()
    spec, peak, full = ps.reduce(d["out_v"], d["out_i"], x["out_i"], flat.R_val, flat.C_val, flat.L_val, tol, freqs, req, full=True)
    assert ps.bits_equal(res["spec"], spec).all() and ps.bits_equal(res["peak"], peak).all() and ps.bits_equal(res["full"], full).all()
    assert lean["full"] is None and ps.bits_equal(lean["spec"], spec).all() and ps.bits_equal(lean["peak"], peak).all()
    assert res["sens_ms"] > 0 and res["kernel_ms"] > 0
    return res, info


@pytest.mark.parametrize("kw,mode", ((dict(threads=64), 2), (dict(no_resident=True), 1), (dict(force_global=True), 1)), ids=("resident", "per_solve", "global"))
def test_run_sens_on_a_handle_equals_the_harness_on_its_own_sweeps(kw, mode):
    """fed_ladder(68, 47), 34 instances x 16 frequencies with phasors of their own, the pair (c30, c4), a window inside the
    sweep: the pass reads the buffers the two sweeps left on the device."""
    flat, freqs, vph = cases.fed_ladder_case()
    flat.out_nodes = np.array([4, 30], np.int32)
    nE = flat.nR + flat.nC + flat.nL
    tol = np.where(np.arange(nE) % 3 == 0, 0.05, 0.01)
    req = abi.ac_sens_req(1, 0, flat.nR, flat.nC, flat.nL, 2, 13)
    res, info = _run_sens_against_its_own_sweeps(flat, freqs, vph, 30, 4, req, tol, kw, mode)
    assert np.isfinite(res["spec"]).all() and (res["spec"][:, :, 2] > 0).all()
    if mode == 1:
        assert (info["lds_bytes"] == 0) == ("force_global" in kw)


def test_run_sens_reads_the_dense_fallback_slots():
    """ladder_case at its resonant frequencies, 64 instances: the near-resonant slots of BOTH sweeps trip the static pivot
    order and are repeated dense before the pass reads them."""
    flat, freqs, vph, near = cases.ladder_case(64)
    flat.out_nodes = np.array([3], np.int32)  # (node b0, between L0 and C0)
    nE = flat.nR + flat.nC + flat.nL
    req = abi.ac_sens_req(0, -1, flat.nR, flat.nC, flat.nL)
    res, info = _run_sens_against_its_own_sweeps(flat, freqs, vph, 3, 0, req, np.full(nE, 0.01), {}, 2)
    assert near.any(axis=1).sum() <= info["tail_levels"] <= near.sum() and info["tail_levels"] > 0, info
    assert np.isfinite(res["spec"]).all()


def test_run_sens_refusals_run_nothing():
    from spicey_amd.lib import AcHandle
    flat, freqs, vph = cases.fed_ladder_case()
    flat.out_nodes = np.array([4, 30], np.int32)
    nE = flat.nR + flat.nC + flat.nL
    tol = np.full(nE, 0.01)
    req = abi.ac_sens_req(1, 0, flat.nR, flat.nC, flat.nL)
    h = AcHandle(flat, interpreter=3)
    r = h.run_sens(freqs, vph, 30, 4, req, tol)
    assert r["status"] == abi.ERR_BAD_DESC and "injection" in r["detail"]
    h.close()
    h = AcHandle(flat)
    for (p, n) in ((0, 0), (5, 5), (flat.n_nodes + 1, 0), (-1, 0)):
        r = h.run_sens(freqs, vph, p, n, req, tol)
        assert r["status"] == abi.ERR_BAD_DESC and "inject" in r["detail"]
    bad = tol.copy()
    bad[-1] = np.inf
    for q, tl in ((abi.ac_sens_req(2, 0, flat.nR, flat.nC, flat.nL), tol), (abi.ac_sens_req(1, 0, flat.nR, flat.nC, flat.nL, 5, 16), tol), (req, bad), (req, None),
                  (abi.ac_sens_req(1, 0, flat.nR - 1, flat.nC, flat.nL), tol)):
        r = h.run_sens(freqs, vph, 30, 4, q, tl)
        assert r["status"] == abi.ERR_BAD_DESC and "sens" in r["detail"], r["detail"]
        assert (r["spec"] == 0).all() and (r["peak"] == 0).all()
    h.close()


def test_a_singular_instance_keeps_its_code_while_the_others_finish():
    """sing_case: the instance whose inductor stamps nothing fails in sweep D (and in X: the matrix is the same); the merged
    table names it, the other instances' rows are those of a handle without it."""
    from spicey_amd.lib import AcHandle
    flat, freqs, vph, flat_ok, vph_ok = cases.sing_case()
    nE = flat.nR + flat.nC + flat.nL
    for f in (flat, flat_ok):
        f.out_nodes = np.array([2], np.int32)
    req = abi.ac_sens_req(0, -1, flat.nR, flat.nC, flat.nL)
    tol = np.full(nE, 0.02)
    h = AcHandle(flat, no_resident=True)
    res = h.run_sens(freqs, vph, 2, 0, req, tol)
    mode = h.info()["interpreter"]
    h.close()
    assert mode == 1 and res["status"] == abi.ERR_SINGULAR
    bad = np.nonzero(res["inst_status"])[0]
    assert bad.tolist() == [cases.SING_AT] and res["inst_status"][cases.SING_AT] == abi.ERR_SINGULAR
    h = AcHandle(flat_ok, no_resident=True)
    ok = h.run_sens(freqs, vph_ok, 2, 0, req, tol)
    h.close()
    assert ok["status"] == 0
    keep = np.arange(flat.n_inst) != cases.SING_AT
    assert ps.bits_equal(res["spec"][keep], ok["spec"]).all() and ps.bits_equal(res["peak"][keep], ok["peak"]).all()


def _same(one, other, k):
    assert list(one) == list(other)
    for key in one:
        a, b = one[key], other[key]
        if key == "elements":
            assert list(a) == list(b) and all(list(a[n].values()) == list(b[n].values()) for n in a), (k, key)
        elif isinstance(a, dict):
            assert list(a) == list(b) and all(np.asarray(a[n]).tobytes() == np.asarray(b[n]).tobytes() for n in a), (k, key)
        else:
            assert np.asarray(a).tobytes() == np.asarray(b).tobytes(), (k, key)


LADDER3 = "V1 in 0 AC 1\nR1 in a 1000\nC1 a 0 1e-9\nR2 a out 2200\nC2 out 0 4.7e-10\nR3 out 0 1e5\n.ac dec 3 1e3 1e7\n.end\n"


def test_batch_of_34_variants_equals_34_single_calls():
    """simulateSensBatch of 34 variants of a two-stage R-C filter is ONE launch, and every slot is bit for bit what
    simulateSens gives for the circuit alone.  34 x 13 slots stay in the per-solve kernel, the kernel of a single circuit: a
    slot's solves and the reduction of an instance do not depend on the rest of the batch."""
    from spicey_amd.lib import HipBackend
    ckts = [parseNetlist(variant(LADDER3, k)) for k in range(34)]
    kw = dict(tol={"R": 0.01, "C": 0.05, "r3": 0.001}, f_from=1e4, f_to=1e6, full=True)
    be = HipBackend()
    res = simulateSensBatch(ckts, "v(out)", backend=be, **kw)
    assert be.ac_launches == [34] and be.info["interpreter"] == 1 and len(res[0]["freqs"]) == 13, (be.ac_launches, be.info)
    for k, c in enumerate(ckts):
        one_be = HipBackend()
        one = simulateSens(c, "v(out)", backend=one_be, **kw)
        assert one_be.info["interpreter"] == 1 and one_be.ac_launches == [1]
        _same(one, res[k], k)
    assert res[0]["elements"]["R3"]["tol"] == 0.001 and list(res[0]["elements"])[-1] == "R3"


def test_rc_closed_form_through_the_public_api():
    """H = 1 / (1 + jwRC): S_R / H = S_C / H = -jwRC / (1 + jwRC), at 3e-9 |ref| + 1e-12."""
    from spicey_amd.lib import HipBackend
    rc = "V1 in 0 AC 1\nR1 in out 1000\nC1 out 0 1e-9\n.ac dec 5 1e3 1e7\n.end\n"
    be = HipBackend()
    r = simulateSens(parseNetlist(rc), "v(out)", tol={"R1": 0.01, "C1": 0.05}, full=True, backend=be)
    assert be.info["interpreter"] == 1 and be.ac_launches == [1]
    w = 2 * np.pi * np.array(r["freqs"])
    ref = -1j * w * 1e-6 / (1 + 1j * w * 1e-6)

    def close(got, want):
        return (np.abs(got - want) <= 3e-9 * np.abs(want) + 1e-12).all()
    for n in ("R1", "C1"):
        assert close(np.array(r["mag_sens"][n]) + 1j * np.radians(np.array(r["phase_sens_deg"][n])), ref), n
    assert close(np.array(r["h"]), 1 / (1 + 1j * w * 1e-6))
    assert close(np.array(r["mag_wc"]), 0.06 * np.abs(ref.real)) and close(np.array(r["mag_sigma"]), np.hypot(0.01, 0.05) * np.abs(ref.real))
    assert list(r["elements"]) == ["C1", "R1"] and r["elements"]["C1"]["f_mag_peak"] == r["freqs"][-1]
    with pytest.raises(ValueError, match="exact_order"):
        simulateSens(parseNetlist(rc), "v(out)", exact_order=True)


@pytest.mark.parametrize("kw,mode", ((dict(threads=64), 2), (dict(no_resident=True), 1), (dict(force_global=True), 1)), ids=("resident", "per_solve", "global"))
def test_plain_sweep_before_and_after_a_sens_run_keeps_its_bits(kw, mode):
    from spicey_amd.lib import AcHandle
    flat, freqs, vph = cases.fed_ladder_case()
    nE = flat.nR + flat.nC + flat.nL
    h = AcHandle(flat, **kw)
    before = h.run(freqs, vph)
    assert before["status"] == 0 and h.info()["interpreter"] == mode
    mid = h.run_sens(freqs, vph, 9, 40, abi.ac_sens_req(8, 39, flat.nR, flat.nC, flat.nL), np.full(nE, 0.01))
    assert mid["status"] == 0 and h.info()["interpreter"] == mode
    after = h.run(freqs, vph)
    h.close()
    assert after["status"] == 0
    assert np.array_equal(before["out_v"], after["out_v"]) and np.array_equal(before["out_i"], after["out_i"])
    # H of the sens run is the plain sweep's own v(9) - v(40)
    hd = before["out_v"][:, :, 8] - before["out_v"][:, :, 39]
    assert ps.bits_equal(mid["spec"][:, :, 0], hd.real).all() and ps.bits_equal(mid["spec"][:, :, 1], hd.imag).all()
