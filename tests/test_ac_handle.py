"""One SpiceyAcHandle for both AC engines (spicey_amd/csrc/ac_abi.cpp): what spicey_ac_create refuses without a device, in
its order, and a handle that serves several calls in a row — every answer that of a fresh handle."""
import ctypes as C

import numpy as np
import pytest

from conftest import bits_equal, golden_netlist, load_golden
from spicey_amd import abi
from spicey_amd.ac_measure import make_ac_reqs
from spicey_amd.netlist import parseNetlist
from test_oracle_ac import cplx

ENGINES = [0, 3]  # SpiceyOptions.interpreter: the sparse engine, the reference-order engine


def _ac_rlc():
    g = load_golden("ac_rlc")
    return abi.flatten(parseNetlist(golden_netlist(g))), np.array(g["freqs"]), cplx(g["vph"])


@pytest.mark.parametrize("interpreter", ENGINES)
def test_ac_create_refusals_without_a_device(interpreter):
    """The descriptor is judged before the device is looked for: (2) for a wrong abi_version, then (4) for a valid one."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from spicey_amd import lib
    L = lib.load()
    flat = _ac_rlc()[0]
    opt = abi.SpiceyOptions()
    opt.interpreter = interpreter
    for bump, code, text in ((1, abi.ERR_BAD_DESC, "abi_version mismatch"), (0, 4, "no HIP device: libspicey_hip has no CPU path")):
        d = flat.desc()
        d.abi_version += bump
        h = C.c_void_p()
        assert L.spicey_ac_create(C.byref(d), C.byref(opt), C.byref(h)) == code
        assert h.value is None and L.spicey_ac_last_error(None).decode() == text


@pytest.mark.gpu
@pytest.mark.parametrize("interpreter", ENGINES)
def test_one_handle_serves_a_sequence_of_calls(interpreter):
    from spicey_amd.lib import AcHandle
    flat, freqs, vph = _ac_rlc()
    n_cur = flat.nR + flat.nC + flat.nL + flat.nV
    # |V| extrema of the last node, a crossing of a current's magnitude, a quotient of two nodes
    reqs = make_ac_reqs([(0, flat.n_out - 1, -1, -1, 0, 0, 0, abi.AC_MEAS_EXTREMA, 0, -1, 0.0, 0, 0, 0),
                         (1, n_cur - 1, -1, -1, 0, 0, 0, abi.AC_MEAS_CROSS, 0, -1, 1e-3, 0, 0, 0),
                         (0, flat.n_out - 1, -1, 0, 0, -1, 0, abi.AC_MEAS_CROSS, 0, -1, 0.5 ** 0.5, 0, 0, 1)])
    refused = make_ac_reqs([(0, flat.n_out, -1, -1, 0, 0, 0, abi.AC_MEAS_EXTREMA, 0, -1, 0.0, 0, 0, 0)])  # column n_out: none

    def fresh(call):
        h = AcHandle(flat, interpreter=interpreter)
        try:
            return call(h)
        finally:
            h.close()

    def same(got, want):
        assert got["status"] == want["status"] == 0
        for k in ("out_v", "out_i", "meas"):
            assert (k in got) == (k in want)
            if k in got:
                assert bits_equal(got[k].view(np.float64), want[k].view(np.float64)).all(), k
        assert (got["inst_status"] == want["inst_status"]).all() and (got["first_freq"] == want["first_freq"]).all()

    calls = [lambda h: h.run(freqs[:5], vph), lambda h: h.run(freqs, vph), lambda h: h.run_measure(freqs, vph, reqs)]
    h = AcHandle(flat, interpreter=interpreter)
    try:
        for call in calls:
            got = call(h)
            same(got, fresh(call))
            assert got["kernel_ms"] > 0
        if interpreter == 3:
            assert h.info()["interpreter"] == 3
        empty = h.run(freqs[:0], vph)
        assert empty["status"] == 0 and (empty["inst_status"] == 0).all() and (empty["first_freq"] == -1).all()
        bad = h.run_measure(freqs, vph, refused)
        assert bad["status"] == abi.ERR_BAD_DESC and bad["measure_ms"] == 0 and (bad["inst_status"] == abi.ERR_BAD_DESC).all()
        again = h.run(freqs, vph)
        same(again, fresh(calls[1]))
        assert again["kernel_ms"] > 0
    finally:
        h.close()
