"""Every refusal of spicey_run_pss on the GPU: SPICEY_ERR_BAD_DESC with its "pss: " text, nothing run, and the handle usable
afterwards — a following plain run gives the bits a fresh handle gives."""
import ctypes as C

import numpy as np
import pytest

import pss_cases as pc
from spicey_amd import abi, pss
from spicey_amd.netlist import parseNetlist

pytestmark = pytest.mark.gpu


def _handle(name, n_inst):
    from spicey_amd.lib import Handle
    ckt = parseNetlist(pc.NETLISTS[name])
    dt, _ = abi.computeEffectiveTimeStep(ckt.analyses["tran"]["dt"], ckt.analyses["tran"]["tstop"])
    m = pc.STEPS_PER_PERIOD[name]
    flat = abi.flatten(ckt).replicate(n_inst)
    return Handle(flat), flat, m, dt, pss.period_table(ckt, dt, m)


def test_every_refusal_names_itself_and_leaves_the_handle_usable():
    h, flat, m, dt, src = _handle("PSS_BOOST", 4)  # nX = 3: W = 4, one circuit
    fresh, *_ = _handle("PSS_BOOST", 4)
    try:
        want = fresh.run(m - 1, dt, src)
        cases = [(dict(n_ckt=2), {}, "instances"), (dict(method=abi.PSS_SETTLE), {}, "instances"), (dict(max_iter=0), {}, "max_iter"), ({}, dict(m_steps=0), "m_steps"),
                 (dict(reltol=0.0), {}, "tolerances"), (dict(vabstol=-1.0), {}, "tolerances"), (dict(iabstol=0.0), {}, "tolerances"), (dict(rel_step=0.0), {}, "rel_step"),
                 (dict(v_scale=0.0), {}, "rel_step"), (dict(i_scale=-1.0), {}, "rel_step"), (dict(damping=0.0), {}, "damping"), (dict(damping=2.0), {}, "damping")]
        for kw, call, text in cases:
            r = h.run_pss(call.get("m_steps", m), dt, src, abi.pss_req(**{"n_ckt": 1, **kw}))
            assert r["status"] == abi.ERR_BAD_DESC and r["detail"].startswith("pss: ") and text in r["detail"], (kw, call, r["detail"])
        for field, bad, text in (("struct_bytes", 80, "struct_bytes"), ("reserved", 1, "reserved"), ("pad", 1, "reserved"), ("method", 7, "unknown method")):
            req = abi.pss_req(1)
            setattr(req, field, bad)
            r = h.run_pss(m, dt, src, req)
            assert r["status"] == abi.ERR_BAD_DESC and r["detail"].startswith("pss: ") and text in r["detail"], (field, r["detail"])
        # null buffers, straight at the C function
        L, req = h.L, abi.pss_req(1)
        x, on, hist = np.zeros((1, 3)), np.zeros((1, 1), np.int32), np.zeros((20, 1, 8))
        n_iter, st = np.zeros(1, np.int32), np.zeros(1, np.int32)
        f64, i32 = C.POINTER(C.c_double), C.POINTER(C.c_int32)
        args = [src.ctypes.data_as(f64), 0, C.addressof(req), x.ctypes.data_as(f64), on.ctypes.data_as(i32), hist.ctypes.data_as(f64), n_iter.ctypes.data_as(i32),
                st.ctypes.data_as(i32)]
        for k in (0, 2, 3, 4, 5, 6, 7):
            a = list(args)
            a[k] = None
            assert L.spicey_run_pss(h.h, m, dt, *a) == abi.ERR_BAD_DESC and h.error().startswith("pss: "), k
        a = list(args)
        a[1] = 2
        assert L.spicey_run_pss(h.h, m, dt, *a) == abi.ERR_BAD_DESC and "src_per_inst" in h.error()
        assert (x == 0).all() and (hist == 0).all()
        got = h.run(m - 1, dt, src)
        assert got["status"] == abi.OK
        for k in ("out_v", "out_i"):
            assert (got[k].view(np.int64) == want[k].view(np.int64)).all(), k
        for k in ("C_vprev", "L_iprev", "D_vdprev", "S_ison"):
            assert (got["state"][k] == want["state"][k]).all(), k
    finally:
        h.close()
        fresh.close()


def test_too_many_states_and_none_are_refused():
    from spicey_amd.lib import Handle
    # 129 capacitors: a ladder
    n = 129
    lines = ["V1 n0 0 PULSE(0 1 0 1u 1u 20u 40u)"] + [f"R{k} n{k} n{k + 1} 1k\nC{k} n{k + 1} 0 1n" for k in range(n)] + [".tran 1u 40u"]
    ckt = parseNetlist("\n".join(lines) + "\n")
    flat = abi.flatten(ckt)
    flat.out_nodes = np.array([1], np.int32)
    src = pss.period_table(ckt, 1e-6, 40)
    h = Handle(flat)
    try:
        r = h.run_pss(40, 1e-6, src, abi.pss_req(1))
        assert r["status"] == abi.ERR_BAD_DESC and r["detail"].startswith("pss: ") and 'method = "settle"' in r["detail"]
        r = h.run_pss(40, 1e-6, src, abi.pss_req(1, abi.PSS_SETTLE, max_iter=2))  # W = 1: the same handle settles
        assert r["status"] == abi.OK and r["history"].shape == (2, 1, 8) and (r["ckt_status"] == abi.PSS_MAX_ITER).all() and (r["history"][:, 0, 0] > 1.0).all() and (r["n_iter"] == 2).all()
    finally:
        h.close()
    none = parseNetlist("V1 in 0 PULSE(0 1 0 1u 1u 20u 40u)\nR1 in out 1k\nR2 out 0 1k\n.tran 1u 40u\n")
    h = Handle(abi.flatten(none))
    try:
        r = h.run_pss(40, 1e-6, pss.period_table(none, 1e-6, 40), abi.pss_req(1))
        assert r["status"] == abi.ERR_BAD_DESC and "no state" in r["detail"]
    finally:
        h.close()
