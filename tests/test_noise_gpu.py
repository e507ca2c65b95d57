"""Noise analysis on the GPU: the injected AC sweep against the CPU harness (tests/noise_host) on the three paths a solve can
take, spicey_ac_noise_device bit for bit against the harness, simulateNoiseBatch against single calls, the RC closed form
through the public API, and an un-injected sweep around an injected one.  Every test asserts which kernel ran.

Bar: |z - z_ref| <= 1e-9 |z_ref| + 1e-12 (ac_resident_cases.py)."""
import numpy as np
import pytest

import ac_resident_cases as cases
from ac_resident_cases import cratio, worst
from batch_variants import variant
from noise_host import pynoise as pn
from spicey_amd import abi
from spicey_amd.netlist import parseNetlist
from spicey_amd.noise import kt4_of, reduce_reference_noise, simulateNoise, simulateNoiseBatch

pytestmark = pytest.mark.gpu

KT4 = kt4_of(300.15)
RC = "V1 in 0 AC 1\nR1 in out 1000\nC1 out 0 1e-9\n.ac dec 5 1e3 1e7\n.end\n"


# (the tests on torch tensors come first: in a process that runs this file alone torch has to open the device before the
# library does, spicey_amd/lib.py load())
def _device_noise(out_v, out_i, R, freqs, req):
    """spicey_ac_noise_device on torch tensors; the results back on the host."""
    import torch

    from spicey_amd import lib
    ni, nf, n_v = out_v.shape
    nR = R.shape[1]
    d_v = torch.from_numpy(np.ascontiguousarray(out_v)).cuda()
    d_i = torch.from_numpy(np.ascontiguousarray(out_i)).cuda()
    d_R = torch.from_numpy(np.ascontiguousarray(R)).cuda()
    d_f = torch.from_numpy(np.ascontiguousarray(freqs)).cuda()
    nan = float("nan")
    d_spec = torch.full((ni, nf, abi.NOISE_SPEC), nan, dtype=torch.float64, device="cuda")
    d_con = torch.full((ni, nR), nan, dtype=torch.float64, device="cuda")
    d_tot = torch.full((ni, 2), nan, dtype=torch.float64, device="cuda")
    need = lib.ac_noise_workspace_bytes(ni, nf, nR)
    d_work = torch.zeros(max(need, 8), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    try:
        lib.ac_noise_device(ni, nf, d_v.data_ptr(), n_v, d_i.data_ptr(), out_i.shape[2], d_R.data_ptr(), nR, d_f.data_ptr(), req, d_spec.data_ptr(),
                            d_con.data_ptr(), d_tot.data_ptr(), d_work.data_ptr(), need)
    finally:
        torch.cuda.synchronize()
    return d_spec.cpu().numpy(), d_con.cpu().numpy(), d_tot.cpu().numpy()


@pytest.mark.parametrize("nR", pn.REDUCTION_NR)
def test_noise_device_equals_the_cpu_harness_bit_for_bit(nR):
    """The reduction shapes of test_noise_host.py: nR around the wave size, one, two and 17 frequencies, three instances, the
    three windows, with and without an input, a frequency whose gain2 is 0."""
    for nf in pn.REDUCTION_NF:
        out_v, out_i, R, freqs = pn.noise_inputs(3, nf, nR, 4, 3, seed=1000 * nR + nf)
        in_col = nR + 2
        out_i[:, nf // 2, in_col] = 0.0
        for (k0, k1) in sorted({(0, -1), (nf // 2, nf // 2), (max(nf - 2, 0), nf - 1)}):
            for (op, on, ic) in ((1, -1, in_col), (0, 2, in_col), (-1, 1, -1)):
                req = abi.ac_noise_req(op, on, ic, KT4, k0, k1)
                got = _device_noise(out_v, out_i, R, freqs, req)
                host = pn.reduce(out_v, out_i, R, freqs, req)
                ref = reduce_reference_noise(out_v, out_i, R, freqs, KT4, op, on, ic, k0, k1)
                for g, h, r, what in zip(got, host, ref, ("spec", "contrib", "total")):
                    assert pn.bits_equal(g, h).all() and pn.bits_equal(g, r).all(), (what, nR, nf, k0, k1, op, on, ic)


def test_noise_device_refusal_launches_nothing():
    import torch

    from spicey_amd import lib
    from spicey_amd.lib import SpiceyNativeError
    out_v, out_i, R, freqs = pn.noise_inputs(2, 5, 7, 2, 2, seed=7)
    d = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (out_v, out_i, R, freqs)]
    outs = [torch.full(s, 7.0, dtype=torch.float64, device="cuda") for s in ((2, 5, 4), (2, 7), (2, 2))]
    need = lib.ac_noise_workspace_bytes(2, 5, 7)
    d_work = torch.zeros(need, dtype=torch.uint8, device="cuda")
    for req, wb in ((abi.ac_noise_req(2, -1, -1, KT4), need), (abi.ac_noise_req(0, 0, -1, KT4), need), (abi.ac_noise_req(0, -1, -1, KT4, 3, 2), need),
                    (abi.ac_noise_req(0, -1, -1, KT4), need - 8)):
        with pytest.raises(SpiceyNativeError) as e:
            lib.ac_noise_device(2, 5, d[0].data_ptr(), 2, d[1].data_ptr(), 9, d[2].data_ptr(), 7, d[3].data_ptr(), req, outs[0].data_ptr(), outs[1].data_ptr(),
                                outs[2].data_ptr(), d_work.data_ptr(), wb)
        assert e.value.status == abi.ERR_BAD_DESC and "noise" in str(e.value)
    torch.cuda.synchronize()
    assert all((o.cpu().numpy() == 7.0).all() for o in outs) and (d_work.cpu().numpy() == 0).all()
    assert lib.ac_noise_workspace_bytes(0, 5, 7) == -1


def injected(flat, freqs, node_p, node_n, vph=None, amp=1.0, **kw):
    """(result, info) of one injected sweep on a handle of its own."""
    from spicey_amd.lib import AcHandle
    h = AcHandle(flat, **kw)
    got = h.run_inject(freqs, vph, node_p, node_n, amp)
    info = h.info()
    h.close()
    return got, info


def test_injected_sweep_in_the_resident_kernel():
    """fed_ladder(68, 47), 34 instances x 16 frequencies on 64 threads: the injected row is beyond the first rows of the
    workgroup for node c66 and among them for c3; a differential pair; an amplitude that is not 1; the source's own node c47,
    whose pivot row is not its pivot column; phasors left on."""
    flat, freqs, vph = cases.fed_ladder_case()
    from random_circuits import fed_ladder
    ckt = parseNetlist(fed_ladder(*cases.FED_LADDER))
    for (p, n, amp, ph) in ((ckt.nodes.get("c3"), 0, 1.0, None), (ckt.nodes.get("c66"), ckt.nodes.get("c20"), 0.5 - 2.0j, None),
                            (0, ckt.nodes.get("c47"), 1.0, None), (ckt.nodes.get("c10"), 0, 1e-3, vph)):
        got, info = injected(flat, freqs, p, n, ph, amp, threads=64)
        assert got["status"] == 0, got["detail"]
        assert info["interpreter"] == 2 and info["threads"] == 64 and info["resident_tasks"] > 0, info
        ref = pn.sweep(flat, freqs, ph, p, n, amp, T=64, resident=True)
        assert ref["status"] == 0
        ev, ei = worst(got, ref)
        print(f"resident, inject {p} -> {n}: {ev:.3g} / {ei:.3g} of the bar, rows {ref['pos']}")
        assert ev <= 1.0 and ei <= 1.0
        assert np.abs(got["out_i"]).max() > 0  # (c47 is held by V1: drawing from it moves the source's current alone)


def test_injected_sweep_in_the_global_workspace_kernel():
    """The same batch with force_global: one workgroup per slot, workspace in global memory."""
    flat, freqs, _ = cases.fed_ladder_case()
    for (p, n) in ((4, 0), (67, 21)):
        got, info = injected(flat, freqs, p, n, force_global=True)
        assert got["status"] == 0, got["detail"]
        assert info["interpreter"] == 1 and info["lds_bytes"] == 0, info
        ref = pn.sweep(flat, freqs, None, p, n, 1.0, T=64)
        ev, ei = worst(got, ref)
        print(f"global workspace, inject {p} -> {n}: {ev:.3g} / {ei:.3g} of the bar")
        assert ev <= 1.0 and ei <= 1.0
    lds, info = injected(flat, freqs, 4, 0, no_resident=True)
    assert lds["status"] == 0 and info["interpreter"] == 1 and info["lds_bytes"] > 0
    assert max(worst(lds, pn.sweep(flat, freqs, None, 4, 0, 1.0, T=64))) <= 1.0


def test_injected_sweep_reaches_the_dense_fallback():
    """ladder_case at its resonant frequencies, 64 instances: the near-resonant slots trip the static pivot order and are
    repeated dense, with the injection in their right-hand side."""
    flat, freqs, _, near = cases.ladder_case(64)
    out = 3  # (node b0, between L0 and C0)
    got, info = injected(flat, freqs, out, 0)
    assert got["status"] == 0, got["detail"]
    assert info["interpreter"] == 2 and near.any(axis=1).sum() <= info["tail_levels"] <= near.sum() and info["tail_levels"] > 0, info
    ref = pn.sweep(flat, freqs, None, out, 0, 1.0, T=64, resident=True)
    assert ref["status"] == 0 and ref["dense"] > 0
    ev, ei = worst(got, ref)
    print(f"dense fallback: {ev:.3g} / {ei:.3g} of the bar, dense solves {info['tail_levels']} (host {ref['dense']})")
    assert ev <= 1.0 and ei <= 1.0
    assert np.abs(got["out_v"][:, :, out - 1][near]).min() > 0  # (the driving-point impedance at the injected node)


def test_run_noise_on_a_handle_equals_the_harness_on_its_own_sweep():
    """AcHandle.run_noise against run_inject on the same handle reduced by the harness, bit for bit (the pass reads the
    buffers the sweep left on the device), in the resident and the per-solve kernel; the interpreter = 3 handle refuses."""
    from spicey_amd.lib import AcHandle
    flat, freqs, _ = cases.fed_ladder_case()
    flat.out_nodes = np.array([4, 30], np.int32)
    in_col = flat.nR + flat.nC + flat.nL
    req = abi.ac_noise_req(1, 0, in_col, KT4, 2, 13)
    for kw, mode in ((dict(threads=64), 2), (dict(no_resident=True), 1)):
        h = AcHandle(flat, **kw)
        res = h.run_noise(freqs, 30, 4, req)
        assert res["status"] == 0 and h.info()["interpreter"] == mode, (res["detail"], h.info())
        sw = h.run_inject(freqs, None, 30, 4)
        assert sw["status"] == 0 and h.info()["interpreter"] == mode
        spec, contrib, total = pn.reduce(sw["out_v"], sw["out_i"], flat.R_val, freqs, req)
        assert pn.bits_equal(res["spec"], spec).all() and pn.bits_equal(res["contrib"], contrib).all() and pn.bits_equal(res["total"], total).all()
        assert np.array_equal(res["gain"], sw["out_i"][:, :, in_col]) and res["noise_ms"] > 0
        h.close()
    h = AcHandle(flat, interpreter=3)
    r = h.run_noise(freqs, 30, 4, req)
    assert r["status"] == abi.ERR_BAD_DESC and "injection" in r["detail"]
    r = h.run_inject(freqs, None, 30, 4)
    assert r["status"] == abi.ERR_BAD_DESC
    h.close()
    h = AcHandle(flat)
    for (p, n) in ((0, 0), (5, 5), (flat.n_nodes + 1, 0), (-1, 0)):
        assert h.run_inject(freqs, None, p, n)["status"] == abi.ERR_BAD_DESC
    assert h.run_noise(freqs, 30, 4, abi.ac_noise_req(2, 0, in_col, KT4))["status"] == abi.ERR_BAD_DESC  # (column out of range: nothing runs)
    h.close()


def _same(one, other, k):
    assert list(one) == list(other)
    for key in one:
        a, b = one[key], other[key]
        if isinstance(a, dict):
            assert list(a) == list(b) and list(a.values()) == list(b.values()), (k, key)
        else:
            assert np.asarray(a).tobytes() == np.asarray(b).tobytes(), (k, key)


LADDER3 = "V1 in 0 AC 1\nR1 in a 1000\nC1 a 0 1e-9\nR2 a out 2200\nC2 out 0 4.7e-10\nR3 out 0 1e5\n.ac dec %d 1e3 1e7\n.end\n"


def test_batch_of_34_variants_equals_34_single_calls():
    """simulateNoiseBatch of 34 variants of a two-stage R-C filter is ONE launch, and every slot is bit for bit what
    simulateNoise gives for the circuit alone.  34 x 13 slots stay in the per-solve kernel, the kernel of a single circuit: a
    slot's solve and the reduction of an instance do not depend on the rest of the batch.  (A batch that outnumbers the CUs
    runs the resident kernel, whose rounding differs from the per-solve kernel's: the second half holds such a batch to the
    parity bar.)"""
    from spicey_amd.lib import HipBackend
    ckts = [parseNetlist(variant(LADDER3 % 3, k)) for k in range(34)]
    be = HipBackend()
    res = simulateNoiseBatch(ckts, "v(out)", input="V1", f_from=1e4, f_to=1e6, backend=be)
    assert be.ac_launches == [34] and be.info["interpreter"] == 1, (be.ac_launches, be.info)
    for k, c in enumerate(ckts):
        one_be = HipBackend()
        one = simulateNoise(c, "v(out)", input="V1", f_from=1e4, f_to=1e6, backend=one_be)
        assert one_be.info["interpreter"] == 1 and one_be.ac_launches == [1]
        _same(one, res[k], k)
    big = [parseNetlist(variant(LADDER3 % 4, k)) for k in range(34)]
    be = HipBackend()
    res = simulateNoiseBatch(big, "v(out)", input="V1", backend=be)
    assert be.ac_launches == [34] and be.info["interpreter"] == 2, (be.ac_launches, be.info)
    for k in (0, 17, 33):
        one = simulateNoise(big[k], "v(out)", input="V1", backend=HipBackend())
        for key in ("onoise", "zout", "gain", "inoise"):
            scale = KT4 if key in ("onoise", "inoise") else 1.0
            assert cratio(np.array(res[k][key]) / scale, np.array(one[key]) / scale).max() <= 1.0, (k, key)
        assert abs(res[k]["total"] - one["total"]) <= 1e-9 * one["total"] and list(res[k]["contributions"]) == list(one["contributions"])


def test_rc_closed_form_through_the_public_api():
    from spicey_amd.lib import HipBackend
    be = HipBackend()
    r = simulateNoise(parseNetlist(RC), "v(out)", input="V1", backend=be)
    assert be.info["interpreter"] == 1 and be.ac_launches == [1]
    w = 2 * np.pi * np.array(r["freqs"])
    h = 1.0 / (1.0 + 1j * w * 1e-6)
    assert cratio(np.array(r["zout"]), 1000.0 * h).max() <= 1.0
    assert cratio(np.array(r["gain"]), h).max() <= 1.0
    assert cratio(np.array(r["onoise"]) / KT4, 1000.0 / (1.0 + (w * 1e-6) ** 2)).max() <= 1.0
    assert cratio(np.array(r["inoise"]) / KT4, np.full(len(w), 1000.0)).max() <= 1.0
    host = simulateNoise(parseNetlist(RC), "v(out)", input="V1", backend=pn.HostNoiseBackend())
    assert cratio(np.array(r["onoise"]) / KT4, np.array(host["onoise"]) / KT4).max() <= 1.0
    assert abs(r["total"] - host["total"]) <= 1e-9 * host["total"] and list(r["contributions"]) == ["R1"]
    with pytest.raises(ValueError, match="exact_order"):
        simulateNoise(parseNetlist(RC), "v(out)", exact_order=True)


@pytest.mark.parametrize("kw,mode", ((dict(threads=64), 2), (dict(no_resident=True), 1), (dict(force_global=True), 1)), ids=("resident", "per_solve", "global"))
def test_plain_sweep_before_and_after_an_injected_one_keeps_its_bits(kw, mode):
    from spicey_amd.lib import AcHandle
    flat, freqs, vph = cases.fed_ladder_case()
    h = AcHandle(flat, **kw)
    before = h.run(freqs, vph)
    assert before["status"] == 0 and h.info()["interpreter"] == mode
    mid = h.run_inject(freqs, vph, 9, 40, 2.0 + 1.0j)
    assert mid["status"] == 0 and h.info()["interpreter"] == mode and not np.array_equal(mid["out_v"], before["out_v"])
    after = h.run(freqs, vph)
    h.close()
    assert after["status"] == 0
    assert np.array_equal(before["out_v"], after["out_v"]) and np.array_equal(before["out_i"], after["out_i"])
    # superposition: the injected run is the plain one plus the injection alone (linear system; at the bar)
    alone, _ = injected(flat, freqs, 9, 40, None, 2.0 + 1.0j, **kw)
    tol = 1e-9 * (np.abs(before["out_v"]) + np.abs(alone["out_v"])) + 1e-12
    assert (np.abs(mid["out_v"] - (before["out_v"] + alone["out_v"])) <= tol).all()
