"""The reference-order engine (SpiceyOptions.interpreter = 3, spicey_amd/csrc/exact.hip) on the GPU: the reference's own
algorithm, bit for bit — against the reference-generated goldens and against the oracle (oracle/spicey_ref.c), in every
workspace layout and thread count, through every layer (C-ABI, Python, TypeScript)."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import (LARGE_GOLDENS, REPO, SINGULAR_GOLDENS, SMALL_GOLDENS, bits_equal, farr, golden_netlist, load_golden)
from spicey_amd import abi
from spicey_amd.netlist import parseNetlist
from spicey_amd.simulate import SingularMatrixError, formatTranResult, simulateTRAN

pytestmark = pytest.mark.gpu


def _flat_run(text, **kw):  # (-> flat, steps, dt, src, result, SpiceyInfo)
    from spicey_amd.lib import HipBackend
    ckt = parseNetlist(text)
    dt, steps = abi.computeEffectiveTimeStep(ckt.analyses["tran"]["dt"], ckt.analyses["tran"]["tstop"])
    flat = abi.flatten(ckt)
    src = abi.source_table(ckt, dt, steps)
    be = HipBackend(interpreter=3, **kw)
    return flat, steps, dt, src, be.run(flat, steps, dt, src), be.info


def _same(a, b):
    assert a["status"] == b["status"], (a["detail"], b["detail"])
    if a["status"] != 0:
        return
    assert np.array_equal(a["iters"], b["iters"])
    assert bits_equal(a["out_v"], b["out_v"]).all() and bits_equal(a["out_i"], b["out_i"]).all()
    for k in ("C_vprev", "L_iprev", "D_vdprev"):
        assert bits_equal(a["state"][k], b["state"][k]).all(), k
    assert np.array_equal(a["state"]["S_ison"], b["state"]["S_ison"])


def _check_golden(name):
    g = load_golden(name)
    ckt = parseNetlist(golden_netlist(g))
    for ri, run in enumerate(g["runs"]):  # run 2 continues from run 1's end state
        res = simulateTRAN(ckt, exact_order=True)
        assert list(res["nodeVoltages"]) == run["keysV"] and list(res["elementCurrents"]) == run["keysI"]
        assert res["times"] == run["times"]
        for k in run["keysV"]:
            assert bits_equal(res["nodeVoltages"][k], farr(run["V"][k])).all(), (name, ri, k)
        for k in run["keysI"]:
            assert bits_equal(res["elementCurrents"][k], farr(run["I"][k])).all(), (name, ri, k)
        assert [c.vPrev for c in ckt.C] == run["state"]["C_vPrev"] and [l.iPrev for l in ckt.L] == run["state"]["L_iPrev"]
        assert [d.vdPrev for d in ckt.D] == run["state"]["D_vdPrev"] and [int(s.isOn) for s in ckt.S] == run["state"]["S_isOn"]
        if ri == 0 and "formatted_head" in run:
            assert formatTranResult(res).split("\n")[:4] == run["formatted_head"]


@pytest.mark.parametrize("name", SMALL_GOLDENS)
def test_small_goldens_bit_exact_in_exact_mode(name):
    _check_golden(name)


@pytest.mark.parametrize("name", ["skip_quirk", "skip_big_c", "skip_clamp_floor", "bridge_rectifier"])
def test_goldens_the_default_path_misses_are_met_bit_for_bit(name):
    """The reference skipped row updates here (or the default path is held to a loose bar): exact mode gives its numbers."""
    _check_golden(name)


@pytest.mark.parametrize("name", LARGE_GOLDENS)
def test_large_goldens_by_hash(name):
    """n ~ 1000: the global slab (one dense n x (n + 1) matrix per instance)."""
    import hashlib
    from spicey_amd.lib import HipBackend
    g = load_golden(name)
    be = HipBackend(interpreter=3)
    res = simulateTRAN(parseNetlist(golden_netlist(g)), backend=be, as_lists=False)
    assert be.info["interpreter"] == 3 and be.info["lds_bytes"] == 0
    assert list(res["nodeVoltages"]) == g["keysV"] and list(res["elementCurrents"]) == g["keysI"]
    V = np.stack([res["nodeVoltages"][k] for k in g["keysV"]], axis=1)
    I = np.stack([res["elementCurrents"][k] for k in g["keysI"]], axis=1)
    assert hashlib.sha256(np.ascontiguousarray(V).tobytes()).hexdigest() == g["sha256_V"]
    assert hashlib.sha256(np.ascontiguousarray(I).tobytes()).hexdigest() == g["sha256_I"]


@pytest.mark.parametrize("name", SINGULAR_GOLDENS)
def test_singular_goldens_raise(name):
    with pytest.raises(SingularMatrixError):
        simulateTRAN(parseNetlist(golden_netlist(load_golden(name))), exact_order=True)


def test_thread_counts_and_workspaces_give_the_same_bits(oracle_backend):
    from spicey_amd import synth
    for text in (golden_netlist(load_golden("bridge_rectifier")), synth.diode_chain(90, seed=3, tran=".tran 1e-6 3e-5")):
        runs = []
        for kw in (dict(threads=64), dict(threads=256), dict(threads=1024), dict(force_global=True), dict(threads=64, force_global=True)):
            flat, steps, dt, src, got, info = _flat_run(text, **kw)
            assert (info["lds_bytes"] == 0) == bool(kw.get("force_global")) and info["threads"] == kw.get("threads", info["threads"])
            runs.append(got)
        ref = oracle_backend.run(flat, steps, dt, src)
        for r in runs:
            _same(r, ref)


def _perturbed(flat, k):
    """A copy of `flat` with every element value scaled by 1 + 0.01 k (k = 0: unchanged)."""
    import copy
    f = copy.deepcopy(flat)
    for a in ("R_val", "C_val", "L_val", "D_is", "S_ron", "S_roff"):
        setattr(f, a, np.ascontiguousarray(getattr(f, a) * (1 + 0.01 * k)))
    return f


def _setup(text):
    ckt = parseNetlist(text)
    dt, steps = abi.computeEffectiveTimeStep(ckt.analyses["tran"]["dt"], ckt.analyses["tran"]["tstop"])
    return abi.flatten(ckt), steps, dt, abi.source_table(ckt, dt, steps)


def test_batches_per_instance_against_the_oracle(oracle_backend):
    """Seven distinct diode_chain(40) instances in one launch, and each skip case stacked with perturbed values: every
    instance bit-equal to the oracle; diagnostics=3 gives the oracle's skip count and lin_err and changes no other bit."""
    from spicey_amd import synth
    from spicey_amd.lib import HipBackend
    batches = []
    flats = [_setup(synth.diode_chain(40, seed=s, tran=".tran 1e-6 2e-5")) for s in range(7)]
    batches.append((abi.stack_instances([f[0] for f in flats]),) + flats[0][1:])
    for name in ("skip_quirk", "skip_big_c", "skip_clamp_floor"):
        flat, steps, dt, src = _setup(golden_netlist(load_golden(name)))
        batches.append((abi.stack_instances([_perturbed(flat, k) for k in range(4)]), steps, dt, src))
    for flat, steps, dt, src in batches:
        got = HipBackend(interpreter=3, diagnostics=3).run(flat, steps, dt, src)
        plain = HipBackend(interpreter=3).run(flat, steps, dt, src)
        ref = oracle_backend.run(flat, steps, dt, src)
        _same(got, ref)
        _same(plain, ref)
        assert np.array_equal(got["skip_risk"], ref["skipped"])
        assert bits_equal(got["lin_err"], ref["lin_err"]).all()


def test_singular_instance_of_a_batch_is_named():
    from spicey_amd.lib import HipBackend
    from spicey_amd import synth
    flat, steps, dt, src = _setup(synth.rc_ladder(10, tran=".tran 1e-6 1e-5"))
    bad = _perturbed(flat, 0)
    bad.R_val = np.ascontiguousarray(bad.R_val * 0 + np.inf)  # every resistor open, every capacitor 0: nothing holds the ladder
    bad.C_val = np.ascontiguousarray(bad.C_val * 0)
    batch = abi.stack_instances([flat, flat, bad, flat])
    got = HipBackend(interpreter=3).run(batch, steps, dt, src)
    assert got["status"] == abi.ERR_SINGULAR and got["detail"].startswith("singular at inst 2 step 0"), got["detail"]


RANDOM_SEEDS = [(s, {}) for s in range(200)] + [(693, dict(floating_sources=True))] + [(s, dict(max_nodes=14)) for s in (467, 2011, 2610, 2833, 2703)]


def test_random_circuits_bit_identical_to_the_oracle(oracle_backend):
    from random_circuits import random_netlist
    from spicey_amd.lib import HipBackend
    for seed, kw in RANDOM_SEEDS:
        flat, steps, dt, src = _setup(random_netlist(seed, **kw))
        got = HipBackend(interpreter=3).run(flat, steps, dt, src)
        ref = oracle_backend.run(flat, steps, dt, src)
        assert got["status"] == ref["status"], (seed, got["detail"], ref["detail"])
        _same(got, ref)


def _hip():
    """The HIP runtime the library itself links (device buffers and a stream of the caller's own)."""
    import ctypes as C
    for name in ("libamdhip64.so", "/opt/rocm/lib/libamdhip64.so"):
        try:
            H = C.CDLL(name)
            break
        except OSError:
            H = None
    assert H is not None
    H.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    H.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    H.hipFree.argtypes = [C.c_void_p]
    H.hipStreamCreate.argtypes = [C.POINTER(C.c_void_p)]
    H.hipStreamDestroy.argtypes = [C.c_void_p]
    return H


def test_run_device_on_a_caller_stream_and_continuation(oracle_backend):
    """spicey_run_device with device buffers on the caller's stream: the bits of spicey_run, and a second run continues
    from the first run's end state."""
    import ctypes as C
    from spicey_amd.lib import Handle
    H = _hip()
    flat, steps, dt, src = _setup(golden_netlist(load_golden("diode_switch")))
    h = Handle(flat, interpreter=3)
    ref = h.run(steps, dt, src)
    ref2 = h.run(steps, dt, src)  # continues from the first run's end state
    h.close()
    _same(ref, oracle_backend.run(flat, steps, dt, src))
    h = Handle(flat, interpreter=3)
    np1 = steps + 1
    sizes = {"src": src.nbytes, "ov": np1 * flat.n_out * 8, "oi": np1 * flat.n_cur * 8, "it": np1 * 4}
    d = {k: C.c_void_p() for k in sizes}
    st = C.c_void_p()
    try:
        for k, nb in sizes.items():
            assert H.hipMalloc(C.byref(d[k]), nb) == 0
        srcc = np.ascontiguousarray(src)
        assert H.hipMemcpy(d["src"], srcc.ctypes.data, sizes["src"], 1) == 0  # host to device
        assert H.hipStreamCreate(C.byref(st)) == 0
        for r in (ref, ref2):
            h.run_device(steps, dt, d["src"].value, d["ov"].value, d["oi"].value, d["it"].value, st.value)
            assert h.sync() == 0, h.error()
            ov, oi, it = np.empty((1, np1, flat.n_out)), np.empty((1, np1, flat.n_cur)), np.empty((1, np1), np.int32)
            for a, k in ((ov, "ov"), (oi, "oi"), (it, "it")):
                assert H.hipMemcpy(a.ctypes.data, d[k], sizes[k], 2) == 0  # device to host
            assert bits_equal(ov, r["out_v"]).all() and bits_equal(oi, r["out_i"]).all() and np.array_equal(it, r["iters"])
    finally:
        h.close()
        if st.value:
            H.hipStreamDestroy(st)
        for v in d.values():
            if v.value:
                H.hipFree(v)


def test_state_get_set_reset():
    from spicey_amd.lib import Handle
    flat, steps, dt, src = _setup(golden_netlist(load_golden("lc_tank")))
    h = Handle(flat, interpreter=3)
    r1 = h.run(steps, dt, src)
    st = h.state()
    r2 = h.run(steps, dt, src)
    h.set_state(st)
    r2b = h.run(steps, dt, src)
    h.reset_state()
    r1b = h.run(steps, dt, src)
    h.close()
    _same(r2, r2b)
    _same(r1, r1b)


def test_multi_handle_matches_single_handle():
    from spicey_amd.lib import HipBackend, MultiHandle
    from spicey_amd import synth
    flats = [_setup(synth.diode_chain(30, seed=s, tran=".tran 1e-6 1e-5")) for s in range(4)]
    flat = abi.stack_instances([f[0] for f in flats])
    steps, dt, src = flats[0][1:]
    one = HipBackend(interpreter=3).run(flat, steps, dt, src)
    m = MultiHandle(flat, [0, 0], interpreter=3)
    assert all(sh["info"]["interpreter"] == 3 for sh in m.shards())
    two = m.run(steps, dt, src)
    m.close()
    _same(one, two)


def test_info_and_refused_options():
    from spicey_amd.lib import Handle, SpiceyNativeError
    flat, steps, dt, src = _setup(golden_netlist(load_golden("dchain20")))
    h = Handle(flat, interpreter=3)
    info = h.info()
    h.close()
    assert info["interpreter"] == 3 and info["threads"] == 64 and info["lds_bytes"] > 0 and info["n_workgroups"] == 1
    assert info["wgs_per_inst"] == 1 and info["inst_per_wg"] == 1 and info["nnz_lu"] == 0 and info["factor_reuse"] == 0
    for kw, word in ((dict(inst_per_wg=2), "inst_per_wg"), (dict(geometry=1), "geometry"), (dict(front_cut=2), "front_cut"),
                     (dict(wgs_per_inst=2), "wgs_per_inst"), (dict(profile=True), "profile")):
        with pytest.raises(SpiceyNativeError, match=word):
            Handle(flat, interpreter=3, **kw)


def test_public_api_guards():
    from spicey_amd.lib import HipBackend
    from spicey_amd.simulate import simulate
    text = golden_netlist(load_golden("skip_quirk"))
    with pytest.raises(ValueError):
        simulateTRAN(parseNetlist(text), backend=HipBackend(), exact_order=True)
    with pytest.raises(ValueError):
        simulate(text, backend=HipBackend(), exact_order=True)
    res = simulate(text, exact_order=True)["tran"]
    assert res["skipRisk"] > 0


@pytest.mark.skipif(shutil.which("node") is None, reason="node not available")
def test_ts_layer_exact_order(tmp_path):
    from test_ts_dropin_node import NODE, _circuit_json, _prepare
    erased, libpath = _prepare(tmp_path)
    g = load_golden("skip_quirk")
    ckt = parseNetlist(golden_netlist(g))
    cj, oj = str(tmp_path / "ckt.json"), str(tmp_path / "out.json")
    json.dump(_circuit_json(ckt), open(cj, "w"))
    r = subprocess.run(NODE + [os.path.join(REPO, "tests", "node", "run_exact.mjs"), erased, cj, oj], capture_output=True, text=True,
                       env=dict(os.environ, SPICEY_HIP_LIB=libpath))
    assert r.returncode == 0, r.stderr
    out = json.load(open(oj))
    assert "error" not in out, out
    t, run = out["tran"], g["runs"][0]
    assert t["keysV"] == run["keysV"] and t["keysI"] == run["keysI"] and t["times"] == run["times"]
    for k in run["keysV"]:
        assert bits_equal(farr(t["V"][k]), farr(run["V"][k])).all(), k
    for k in run["keysI"]:
        assert bits_equal(farr(t["I"][k]), farr(run["I"][k])).all(), k
    assert t["state"]["vdPrev"] == run["state"]["D_vdPrev"] and t["skipRisk"] > 0
