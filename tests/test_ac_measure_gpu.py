"""The AC measurements on the GPU: spicey_ac_measure_device on device tensors against the CPU harness and reduce_ac_reference
(bit for bit, all 8 fields: no field is a sum); its refusals; AcHandle.run_measure in both engines; measureACBatch."""
import numpy as np
import pytest

from ac_measure_host import pyacmeasure as pam
from batch_variants import variant
from conftest import bits_equal, golden_netlist, load_golden
from spicey_amd import abi
from spicey_amd import ac as sac
from spicey_amd.ac_measure import at, extrema, fcross, make_ac_reqs, measureAC, measureACBatch, reduce_ac_reference
from spicey_amd.netlist import parseNetlist
from test_oracle_ac import cplx

pytestmark = pytest.mark.gpu


def _device_measure(out_v, out_i, reqs, work_bytes=None, sentinel=None):
    """spicey_ac_measure_device on torch tensors; the result back on the host."""
    import torch

    from spicey_amd import lib
    ni, nf, n_v = out_v.shape
    d_v = torch.from_numpy(np.ascontiguousarray(out_v)).cuda()
    d_i = torch.from_numpy(np.ascontiguousarray(out_i)).cuda() if out_i is not None else None
    n_req = len(reqs)
    d_meas = torch.full((ni, max(n_req, 1), 8), float("nan") if sentinel is None else sentinel, dtype=torch.float64, device="cuda")
    need = lib.ac_measure_workspace_bytes(ni, nf, max(n_req, 1))
    nbytes = need if work_bytes is None else work_bytes
    d_work = torch.zeros(max(nbytes, 8), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    try:
        lib.ac_measure_device(ni, nf, d_v.data_ptr(), n_v, d_i.data_ptr() if d_i is not None else 0, out_i.shape[2] if out_i is not None else 0,
                              reqs, d_meas.data_ptr(), d_work.data_ptr(), nbytes)
    finally:
        torch.cuda.synchronize()
        host = d_meas.cpu().numpy()
    return host[:, :n_req]


@pytest.mark.parametrize("nv", pam.N_VS)
def test_ac_measure_device_equals_the_cpu_harness_and_the_reference(nv):
    for nf in pam.N_FREQS:
        v, i = pam.buffers(nf, nv, seed=1000 * nf + nv)
        pool = pam.request_pool(nf, nv, pam.N_I, seed=nf + nv)
        full = _device_measure(v, i, pool)
        assert bits_equal(full, pam.run(v, i, pool)).all(), nf
        assert bits_equal(full, reduce_ac_reference(v, i, pool)).all(), nf
        perm = np.random.default_rng(nv).permutation(len(pool))[:60]
        assert bits_equal(_device_measure(v, i, pool[perm]), full[:, perm]).all(), nf
        assert bits_equal(_device_measure(v, i, pool[7:8]), full[:, 7:8]).all(), nf


def test_refusals_return_bad_desc_and_launch_nothing():
    import torch

    from spicey_amd import lib
    from spicey_amd.lib import SpiceyNativeError, ac_measure_workspace_bytes
    nf, nv = 65, 2
    v, i = pam.buffers(nf, nv, seed=3)
    good, bad = pam.refusals(nf, nv, pam.N_I)
    cases = [(i if have_i else None, reqs, None) for _, reqs, have_i in bad]
    cases.append((i, good, ac_measure_workspace_bytes(pam.N_INST, nf, 1) - 8))  # workspace too small
    for oi, reqs, wb in cases:
        with pytest.raises(SpiceyNativeError) as e:
            _device_measure(v, oi, reqs, work_bytes=wb, sentinel=7.0)
        assert e.value.status == abi.ERR_BAD_DESC and "ac measure" in str(e.value), str(e.value)
    # nothing ran: the result buffer and the workspace of a refused call keep what they held
    d_v = torch.from_numpy(v).cuda()
    d_meas = torch.full((pam.N_INST, 2, 8), 7.0, dtype=torch.float64, device="cuda")
    d_work = torch.zeros(ac_measure_workspace_bytes(pam.N_INST, nf, 2), dtype=torch.uint8, device="cuda")
    for _, reqs, have_i in bad[:14]:  # (the lists of two requests: a good one first, so a launch would have written)
        with pytest.raises(SpiceyNativeError):
            lib.ac_measure_device(pam.N_INST, nf, d_v.data_ptr(), nv, 0, 0, reqs, d_meas.data_ptr(), d_work.data_ptr(), d_work.numel())
    torch.cuda.synchronize()
    assert (d_meas.cpu().numpy() == 7.0).all() and (d_work.cpu().numpy() == 0).all()
    assert ac_measure_workspace_bytes(0, nf, 1) == -1
    # and the accepted neighbour of those calls works
    assert bits_equal(_device_measure(v, i, good), reduce_ac_reference(v, i, good)).all()


def _requests_for(n_v, n_i, nf):
    """Extrema of every `what` and crossings on every column, whole sweep and a window, plus quotients against column 0."""
    rows = []
    for sig, n in ((0, n_v), (1, n_i)):
        for col in range(n):
            rows.append((sig, col, -1, -1, 0, 0, col % 3, abi.AC_MEAS_EXTREMA, 0, -1, 0.0, 0, 0, 0))
            rows.append((sig, col, (col + 1) % n if n > 1 else -1, -1, 0, 0, 0, abi.AC_MEAS_EXTREMA, nf // 3, (2 * nf) // 3, 0.0, 0, 0, 0))
            rows.append((sig, col, -1, 0, 0, -1, 0, abi.AC_MEAS_CROSS, 0, -1, 0.5 ** 0.5, (1, -1, 0)[col % 3], col % 2, 1))
            rows.append((sig, col, -1, -1, 0, 0, 1 + col % 2, abi.AC_MEAS_CROSS, 0, -1, 0.0, 0, 1 - col % 2, 0))
            rows.append((sig, col, -1, -1, 0, 0, 0, abi.AC_MEAS_EXTREMA, nf // 2, nf // 2, 0.0, 0, 0, 0))
    return make_ac_reqs(rows)


@pytest.mark.parametrize("name", ["ac_rlc", "ac_two_src", "ac_skip_rc"])
def test_run_measure_in_exact_mode_against_run_and_the_goldens(name):
    from spicey_amd.lib import AcHandle
    g = load_golden(name)
    ckt = parseNetlist(golden_netlist(g))
    flat = abi.flatten(ckt)
    freqs, vph = np.array(g["freqs"]), cplx(g["vph"])
    h = AcHandle(flat, interpreter=3)
    full = h.run(freqs, vph)
    assert full["status"] == 0 and (full["inst_status"] == 0).all() and (full["first_freq"] == -1).all()
    reqs = _requests_for(flat.n_out, flat.nR + flat.nC + flat.nL + flat.nV, len(freqs))
    got = h.run_measure(freqs, vph, reqs)
    h.close()
    assert got["status"] == 0 and got["measure_ms"] > 0 and (got["inst_status"] == 0).all()
    assert bits_equal(got["meas"], reduce_ac_reference(full["out_v"], full["out_i"], reqs)).all()
    # the extrema of |V|^2 of every node: the reference's own numbers (JSON cannot carry the sign of a zero: + 0.0 folds it)
    names = ckt.nodes.rev
    vgold = np.stack([cplx(g["V"][names[n]]) for n in range(1, ckt.nodes.count())], axis=1)[None]
    mag = make_ac_reqs([(0, c, -1, -1, 0, 0, 0, abi.AC_MEAS_EXTREMA, 0, -1, 0.0, 0, 0, 0) for c in range(flat.n_out)])
    h = AcHandle(flat, interpreter=3)
    m = h.run_measure(freqs, vph, mag)["meas"]
    h.close()
    assert bits_equal(m + 0.0, reduce_ac_reference(vgold, None, mag) + 0.0).all()


@pytest.mark.parametrize("name", ["ac_rlc", "ac_two_src", "ac_readme"])
def test_run_measure_on_the_default_engine(name, oracle_backend):
    from spicey_amd.lib import AcHandle
    g = load_golden(name)
    ckt = parseNetlist(golden_netlist(g))
    flat = abi.flatten(ckt)
    freqs, vph = np.array(g["freqs"]), cplx(g["vph"])
    reqs = _requests_for(flat.n_out, flat.nR + flat.nC + flat.nL + flat.nV, len(freqs))
    h = AcHandle(flat)
    full = h.run(freqs, vph)
    got = h.run_measure(freqs, vph, reqs)
    h.close()
    assert full["status"] == 0 and got["status"] == 0
    assert bits_equal(got["meas"], reduce_ac_reference(full["out_v"], full["out_i"], reqs)).all()
    # the H fields against the oracle's, where both picked the same sample (an extreme may tie within rounding elsewhere)
    ref = oracle_backend.run_ac(flat, freqs, vph)
    want = reduce_ac_reference(ref["out_v"], ref["out_i"], reqs)
    ext = np.nonzero((reqs["kind"] == abi.AC_MEAS_EXTREMA) & (reqs["k_from"] == reqs["k_to"]))[0]
    assert len(ext)
    for r in ext:  # point read-outs: the same sample for sure
        zg, zr = complex(*got["meas"][0, r, 4:6]), complex(*want[0, r, 4:6])
        assert abs(zg - zr) <= 1e-9 * abs(zr) + 1e-12
    same = (got["meas"][0, :, 2] == want[0, :, 2]) & (reqs["kind"] == abi.AC_MEAS_EXTREMA)
    assert same.sum() >= len(ext)
    for r in np.nonzero(same)[0]:
        zg, zr = complex(*got["meas"][0, r, 4:6]), complex(*want[0, r, 4:6])
        assert abs(zg - zr) <= 1e-9 * abs(zr) + 1e-12


@pytest.mark.parametrize("exact", [True, False])
def test_measure_ac_batch(exact):
    from spicey_amd.lib import HipAcExactBackend, HipBackend
    good = golden_netlist(load_golden("ac_readme"))
    ts = [variant(good, k) for k in range(8)]
    ts.insert(4, golden_netlist(load_golden("ac_sing_first")))
    measures = {"fc": fcross("v(2)/v(1)", 0.5 ** 0.5), "pk": extrema("v(2)"), "lo": at("v(2)", 10.0)}
    be = HipAcExactBackend() if exact else HipBackend()
    got = measureACBatch([parseNetlist(t) for t in ts], measures, backend=be)
    assert be.ac_launches == [8, 1]  # one handle with the 8 variants as its instances, one for the other topology
    assert isinstance(got[4], sac.SingularComplexMatrixError)
    fcs = []
    for k in (0, 1, 2, 3, 5, 6, 7, 8):
        m = got[k]
        assert list(m) == ["fc", "pk", "lo"] and m["fc"]["count"] == 1 and m["fc"]["f_lo"] <= m["fc"]["f"] <= m["fc"]["f_hi"]
        fcs.append(m["fc"]["f"])
        if exact:
            assert m == measureAC(parseNetlist(ts[k]), measures, exact_order=True)
    assert fcs == sorted(fcs, reverse=True) and abs(fcs[0] - 53.05) < 0.3  # 1 / (2 pi 30 Ohm 100 uF)
