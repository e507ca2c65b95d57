"""Per-instance source tables (SpiceyRun::src_stride) through the kernels' own phase code on the CPU (tests/batch_host):
v1, v2 with K = 1 and K = 2, the hybrid layout and the reference-order engine, every instance against the oracle on its
own table; a per-instance layout whose rows are all equal gives the bits of the shared table."""
import ctypes as C
import os

import numpy as np
import pytest

from batch_variants import PerInstanceOracle
import harness_build
from conftest import REPO, bits_equal
from spicey_amd import abi, synth

HERE = os.path.join(REPO, "tests", "batch_host")
_LIB = None


def lib():
    global _LIB
    if _LIB is None:
        L = harness_build.load(HERE, "libspicey_batch_host.so")
        f64p, i32p = C.POINTER(C.c_double), C.POINTER(C.c_int32)
        L.spicey_batch_emul_run.restype = C.c_int32
        L.spicey_batch_emul_run.argtypes = [C.POINTER(abi.SpiceyDesc), C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int64, C.c_double, f64p, C.c_int64,
                                            f64p, f64p, i32p, f64p, f64p, f64p, i32p, i32p]
        L.spicey_batch_exact_run.restype = C.c_int32
        L.spicey_batch_exact_run.argtypes = [C.POINTER(abi.SpiceyDesc), C.c_int32, C.c_int64, C.c_double, f64p, C.c_int64,
                                             f64p, f64p, i32p, f64p, f64p, f64p, i32p, i32p]
        _LIB = L
    return _LIB


def _p(a, t):
    return a.ctypes.data_as(C.POINTER(t))


def run(flat, steps, dt, src, K=1, T=64, rmax=-1, hybrid=False, exact=False):
    ni = flat.n_inst
    src = np.ascontiguousarray(src, dtype=np.float64)
    stride = (steps + 1) * flat.nV if src.ndim == 3 else 0
    out_v = np.zeros((ni, steps + 1, flat.n_out))
    out_i = np.zeros((ni, steps + 1, flat.n_cur))
    iters = np.zeros((ni, steps + 1), np.int32)
    st = {"C_vprev": flat.C_vprev.copy(), "L_iprev": flat.L_iprev.copy(), "D_vdprev": flat.D_vdprev.copy(), "S_ison": flat.S_ison.copy()}
    status = np.zeros((ni + K - 1) // K * 4, np.int32)
    d = flat.desc()
    tail = (_p(src, C.c_double), stride, _p(out_v, C.c_double), _p(out_i, C.c_double), _p(iters, C.c_int32), _p(st["C_vprev"], C.c_double),
            _p(st["L_iprev"], C.c_double), _p(st["D_vdprev"], C.c_double), _p(st["S_ison"], C.c_int32), _p(status, C.c_int32))
    if exact:
        rc = lib().spicey_batch_exact_run(C.byref(d), T, steps, dt, *tail)
    else:
        rc = lib().spicey_batch_emul_run(C.byref(d), K, T, rmax, int(hybrid), steps, dt, *tail)
    return {"status": rc, "out_v": out_v, "out_i": out_i, "iters": iters, "state": st}


def tol_ratio(got, ref):
    return np.abs(got - ref) / (1e-9 * np.abs(ref) + 1e-12)


def _batch(n=30, ni=5):
    flat, dt, steps, src = synth.chain_batch("diode_chain", n, range(1, ni + 1), tran=".tran 1e-6 1.5e-5")
    tabs = np.ascontiguousarray(np.stack([src * (1.0 - 0.13 * k) for k in range(ni)]))
    return flat, dt, steps, src, tabs


PLANS = {"v1_k1": dict(K=1), "v1_k2": dict(K=2), "v1_k4": dict(K=4), "v2_k1": dict(rmax=6), "v2_k2": dict(K=2, rmax=6),
         "v2_hybrid": dict(rmax=6, hybrid=True), "exact": dict(exact=True)}


@pytest.mark.parametrize("plan", sorted(PLANS))
def test_every_instance_meets_the_oracle_on_its_own_table(plan):
    kw = PLANS[plan]
    flat, dt, steps, src, tabs = _batch()
    got = run(flat, steps, dt, tabs, **kw)
    assert got["status"] == 0
    ref = PerInstanceOracle().run(flat, steps, dt, tabs)
    assert np.array_equal(got["iters"], ref["iters"])
    if kw.get("exact"):
        assert bits_equal(got["out_v"], ref["out_v"]).all() and bits_equal(got["out_i"], ref["out_i"]).all()
        assert bits_equal(got["state"]["D_vdprev"], ref["state"]["D_vdprev"]).all()
    else:
        assert tol_ratio(got["out_v"], ref["out_v"]).max() <= 1.0 and tol_ratio(got["out_i"], ref["out_i"]).max() <= 1.0
        assert tol_ratio(got["state"]["C_vprev"], ref["state"]["C_vprev"]).max() <= 1.0
    for j in range(1, flat.n_inst):  # each instance saw its own table
        assert not np.array_equal(got["out_v"][j], got["out_v"][0])


@pytest.mark.parametrize("plan", sorted(PLANS))
def test_equal_rows_give_the_bits_of_the_shared_table(plan):
    kw = PLANS[plan]
    flat, dt, steps, src, tabs = _batch()
    shared = run(flat, steps, dt, src, **kw)
    same = run(flat, steps, dt, np.broadcast_to(src, tabs.shape), **kw)
    assert shared["status"] == 0 and same["status"] == 0
    for k in ("out_v", "out_i"):
        assert bits_equal(shared[k], same[k]).all(), k
    assert np.array_equal(shared["iters"], same["iters"])


def test_a_table_per_instance_is_not_the_first_instances_table():
    """Without the stride every instance would read instance 0's table: instance 1 here must differ from a run in which
    all instances take table 0."""
    flat, dt, steps, src, tabs = _batch(ni=2)
    per = run(flat, steps, dt, tabs, K=2)
    first = run(flat, steps, dt, tabs[0], K=2)
    assert np.array_equal(per["out_v"][0], first["out_v"][0]) and not np.array_equal(per["out_v"][1], first["out_v"][1])


def _many_sources(n=80, ni=3):
    """n > T = 64 voltage sources, each driving an RC branch of one coupled ladder: the v2 Z phase records the sources
    beyond the first T in its remainder loop (tran_exec.h, zrem bit 4)."""
    from spicey_amd.netlist import parseNetlist
    lines = ["* more sources than threads"]
    for k in range(n):
        lines += [f"V{k} a{k} 0 PULSE(0 {1 + 0.01 * k!r} 0 1n 1n 5u 10u)", f"R{k} a{k} c{k} {1000 + 10 * k}", f"C{k} c{k} 0 1n"]
        if k:
            lines.append(f"RL{k} c{k - 1} c{k} 100")
    lines.append(".tran 1e-6 1.2e-5")
    ckt = parseNetlist("\n".join(lines) + "\n")
    dt, steps = abi.computeEffectiveTimeStep(ckt.analyses["tran"]["dt"], ckt.analyses["tran"]["tstop"])
    src = abi.source_table(ckt, dt, steps)
    tabs = np.ascontiguousarray(np.stack([src * (1.0 - 0.13 * k) for k in range(ni)]))
    return abi.flatten(ckt).replicate(ni), dt, steps, src, tabs


@pytest.mark.parametrize("plan", ["v1_k1", "v1_k2", "v2_k1", "v2_k2", "exact"])
def test_more_sources_than_threads(plan):
    kw = PLANS[plan]
    flat, dt, steps, src, tabs = _many_sources()
    assert flat.nV > 64
    got = run(flat, steps, dt, tabs, T=64, **kw)
    assert got["status"] == 0
    ref = PerInstanceOracle().run(flat, steps, dt, tabs)
    assert np.array_equal(got["iters"], ref["iters"])
    if kw.get("exact"):
        assert bits_equal(got["out_v"], ref["out_v"]).all() and bits_equal(got["out_i"], ref["out_i"]).all()
    else:
        assert tol_ratio(got["out_v"], ref["out_v"]).max() <= 1.0 and tol_ratio(got["out_i"], ref["out_i"]).max() <= 1.0
    same = run(flat, steps, dt, np.broadcast_to(src, tabs.shape), T=64, **kw)
    shared = run(flat, steps, dt, src, T=64, **kw)
    assert bits_equal(same["out_v"], shared["out_v"]).all() and bits_equal(same["out_i"], shared["out_i"]).all()
