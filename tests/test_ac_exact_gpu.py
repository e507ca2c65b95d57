"""The reference-order AC engine (spicey_ac_create with SpiceyOptions.interpreter = 3, spicey_amd/csrc/ac_exact.hip) on the
GPU: the reference's own solveComplex, bit for bit — against the reference-generated goldens and the oracle
(oracle/spicey_ref_ac.c), in every workspace layout and thread count, through every layer (C-ABI, Python, TypeScript)."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import REPO, golden_netlist, load_golden
from spicey_amd import abi, ac as sac
from spicey_amd.netlist import parseNetlist
from test_ac_exact_host import (ERROR_GOLDENS, SKIP_GOLDENS, Fixed, check_golden_result, first_failing_frequency, hypot_cases, random_ac_case,
                                raw_same, sha_of, v8_hypot)
from test_oracle_ac import AC_SMALL, ac_golden_netlist, cbits, cplx

pytestmark = pytest.mark.gpu


def _run(flat, freqs, vph, **kw):  # (-> result, SpiceyInfo after the run)
    from spicey_amd.lib import AcHandle
    h = AcHandle(flat, interpreter=3, **kw)
    try:
        return h.run(np.asarray(freqs, np.float64), vph), h.info()
    finally:
        h.close()


@pytest.mark.parametrize("name", AC_SMALL + SKIP_GOLDENS)
def test_goldens_bit_exact_through_the_handle(name, oracle_backend):
    from spicey_amd.lib import HipAcExactBackend
    g = load_golden(name)
    ckt = parseNetlist(ac_golden_netlist(g))
    flat, freqs, vph = abi.flatten(ckt), np.array(g["freqs"]), cplx(g["vph"])
    got, info = _run(flat, freqs, vph)
    raw_same(got, oracle_backend.run_ac(flat, freqs, vph))
    assert info["interpreter"] == 3 and info["n_workgroups"] == len(freqs) and info["threads"] == (64 if info["n_var"] <= 64 else 256)
    assert info["lds_bytes"] > 0
    check_golden_result(sac.simulateAC(ckt, backend=Fixed(HipAcExactBackend(), vph), freqs=g["freqs"]), g)


def test_large_golden_sha256_on_the_global_slab():
    from spicey_amd.lib import HipAcExactBackend
    g = load_golden("ac_rc1000")
    ckt = parseNetlist(ac_golden_netlist(g))
    be = HipAcExactBackend()
    res = sac.simulateAC(ckt, backend=Fixed(be, cplx(g["vph"])), freqs=g["freqs"])
    assert be.info["lds_bytes"] == 0 and be.info["threads"] == 256 and be.info["interpreter"] == 3
    for k, v in g["V"].items():
        assert cbits(res["nodeVoltages"][k], cplx(v)), k
    for k, v in g["I"].items():
        assert cbits(res["elementCurrents"][k], cplx(v)), k
    assert sha_of(res, g) == {"sha256_V": g["sha256_V"], "sha256_I": g["sha256_I"]}


@pytest.mark.parametrize("name", AC_SMALL + SKIP_GOLDENS)
def test_public_api_formats_the_goldens(name):
    """simulateAC(ckt, exact_order=True) and simulate(text, ac_exact_order=True), this host's frequency list and phasors."""
    from spicey_amd.simulate import simulate
    g = load_golden(name)
    text = ac_golden_netlist(g)
    assert sac.formatAcResult(sac.simulateAC(parseNetlist(text), exact_order=True)) == g["formatted"]
    out = simulate(text, ac_exact_order=True)
    assert sac.formatAcResult(out["ac"]) == g["formatted"]


@pytest.mark.parametrize("name", ["ac_mesh6", "ac_ladder30", "ac_skip_rc", "ac_rlc"])
def test_threads_and_layouts_give_the_same_bits(name):
    g = load_golden(name)
    flat, freqs, vph = abi.flatten(parseNetlist(ac_golden_netlist(g))), np.array(g["freqs"]), cplx(g["vph"])
    base, _ = _run(flat, freqs, vph)
    for kw in (dict(threads=64), dict(threads=128), dict(threads=256), dict(threads=1024), dict(force_global=True),
               dict(force_global=True, threads=1024)):
        got, info = _run(flat, freqs, vph, **kw)
        raw_same(got, base)
        if kw.get("force_global"):
            assert info["lds_bytes"] == 0
        if "threads" in kw:
            assert info["threads"] == kw["threads"]


def test_batch_of_distinct_instances(oracle_backend):
    """Perturbed copies of one topology in one launch: each instance gets its own oracle result."""
    from spicey_amd import synth
    base = synth.rc_ladder(n=30, seed=4, tran=".ac dec 10 1e3 1e8")
    flats = []
    for k in range(6):
        f = abi.flatten(parseNetlist(base))
        f.R_val = f.R_val * (1 + 0.07 * k)
        f.C_val = f.C_val * (1 - 0.05 * k)
        flats.append(f)
    flat = abi.stack_instances(flats)
    freqs = np.geomspace(1e3, 1e8, 41)
    vph = np.ones(flat.nV, np.complex128)
    got, info = _run(flat, freqs, vph)
    assert got["status"] == 0 and info["n_workgroups"] == 6 * 41
    for k, f in enumerate(flats):
        ref = oracle_backend.run_ac(f, freqs, vph)
        one = {"status": 0, "out_v": got["out_v"][k:k + 1], "out_i": got["out_i"][k:k + 1]}
        raw_same(one, ref)


def test_random_circuits_against_oracle(oracle_backend):
    for seed in range(200):
        flat, freqs, vph = random_ac_case(seed)
        ref = oracle_backend.run_ac(flat, freqs, vph)
        got, _ = _run(flat, freqs, vph)
        raw_same(got, ref)
        if ref["status"] != 0:
            assert got["detail"].endswith(f"at inst 0 frequency index {first_failing_frequency(oracle_backend, flat, freqs, vph)}"), seed


def test_resonance_frequencies_against_oracle(oracle_backend):
    """The frequencies of test_ac_resonance_dense_fallback_on_gpu (where the default path repeats solves with its dense
    fallback): bit for bit; a floating tank stays singular."""
    import math
    from random_circuits import series_rlc_ladder
    flats = [abi.flatten(parseNetlist(series_rlc_ladder(12, l=1e-3 * (1 + 0.25 * k)))) for k in range(4)]
    flat = abi.stack_instances(flats)
    f0 = 1.0 / (2.0 * math.pi * math.sqrt(1e-3 * 1e-6))
    freqs = np.array([f0 * (1.0 + d) for d in (1e-2, 1e-6, 1e-9, 1e-12, 0.0, -1e-10)] + [f0 / math.sqrt(1.25), 777.0])
    vph = np.ones(flat.nV, np.complex128)
    ref = oracle_backend.run_ac(flat, freqs, vph)
    assert ref["status"] == 0
    for kw in (dict(), dict(force_global=True)):
        raw_same(_run(flat, freqs, vph, **kw)[0], ref)
    text = "* floating tank\nV1 in 0 AC 1\nR1 in 0 1k\nL1 a 0 1\nC1 a 0 1\n.ac lin 1 1 1\n.end\n"
    flat = abi.flatten(parseNetlist(text))
    freqs = np.array([1.0 / (2.0 * math.pi)])
    ref = oracle_backend.run_ac(flat, freqs, np.ones(1, np.complex128))
    assert ref["status"] != 0 and _run(flat, freqs, np.ones(1, np.complex128))[0]["status"] == ref["status"]


@pytest.mark.parametrize("name,exc,msg", ERROR_GOLDENS)
def test_error_goldens(name, exc, msg, oracle_backend):
    g = load_golden(name)
    ckt = parseNetlist(golden_netlist(g))
    with pytest.raises(exc, match=msg.replace("(", r"\(").replace(")", r"\)")):
        sac.simulateAC(ckt, exact_order=True)
    freqs = sac.buildFrequencyArray(**{k: g["acSpec"][k] for k in ("mode", "N", "f1", "f2")})
    flat, vph = abi.flatten(ckt), sac.source_phasors(ckt)
    got, _ = _run(flat, freqs, vph)
    assert got["detail"] == f"{msg} at inst 0 frequency index {first_failing_frequency(oracle_backend, flat, freqs, vph)}"


def test_first_failing_slot_and_host_errors():
    from spicey_amd.lib import AcHandle, SpiceyNativeError
    text = "* divide\nV1 1 0 ac 1\nR1 1 2 1k\nL1 2 0 1n\n.ac lin 2 1 2\n.end\n"
    flat = abi.stack_instances([abi.flatten(parseNetlist(text)), abi.flatten(parseNetlist(text.replace("1n", "1e-15")))])
    got, _ = _run(flat, [1e6, 5e5, 1.0], np.ones(1, np.complex128))
    assert got["status"] == abi.ERR_COMPLEX_DIV and got["detail"] == "Complex divide by ~0 at inst 0 frequency index 2"
    with pytest.raises(ValueError, match="R R1 must be > 0"):
        sac.simulateAC(parseNetlist(golden_netlist(load_golden("ac_err_r0"))), exact_order=True)
    for T in (32, 100, 2048):
        with pytest.raises(SpiceyNativeError, match="threads"):
            AcHandle(flat, interpreter=3, threads=T)


def test_public_api_guards():
    from spicey_amd.lib import HipBackend
    from spicey_amd.simulate import simulate
    text = golden_netlist(load_golden("ac_skip_rc"))
    with pytest.raises(ValueError):
        sac.simulateAC(parseNetlist(text), backend=HipBackend(), exact_order=True)
    with pytest.raises(ValueError):
        simulate(text, backend=HipBackend(), ac_exact_order=True)
    out = simulate(text, ac_exact_order=True)
    assert out["tran"] is None and sac.formatAcResult(out["ac"]) == load_golden("ac_skip_rc")["formatted"]


def test_device_hypot_is_v8s(tmp_path):
    """spicey_v8_hypot on the device (a probe compiled like ac_exact.hip) against a restatement of V8's algorithm on 1.2e6
    pairs: near-ties, zeros, subnormals, overflowing squares, Inf and NaN."""
    exe = str(tmp_path / "hypot_probe")
    src = os.path.join(REPO, "tests", "ac_exact_host", "hypot_probe.hip")
    subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-o", exe, src], check=True, timeout=300)
    x, y = hypot_cases(1_200_000, seed=9)
    inp, outp = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    np.stack([x, y], 1).astype(np.float64).tofile(inp)
    subprocess.run([exe, inp, outp], check=True, timeout=120)
    got = np.fromfile(outp, np.float64)
    want = v8_hypot(x, y)
    bad = ~((got.view(np.uint64) == want.view(np.uint64)) | (np.isnan(got) & np.isnan(want)))
    assert not bad.any(), (x[bad][:5], y[bad][:5], got[bad][:5], want[bad][:5])


@pytest.mark.skipif(shutil.which("node") is None, reason="node not available")
def test_ts_layer_exact_order(tmp_path):
    """ts/simulateAC.ts with { exactOrder: true } under Node: the JS engine's own frequency list and phasors, so the skip
    golden comes out bit for bit, frequencies included."""
    from test_ts_dropin_node import NODE, _circuit_json, _prepare
    erased, libpath = _prepare(tmp_path)
    for name in SKIP_GOLDENS:
        g = load_golden(name)
        ckt = parseNetlist(golden_netlist(g))
        cj, oj = str(tmp_path / "ckt.json"), str(tmp_path / "out.json")
        json.dump(_circuit_json(ckt), open(cj, "w"))
        r = subprocess.run(NODE + [os.path.join(REPO, "tests", "node", "run_ac_exact.mjs"), erased, cj, oj], capture_output=True, text=True,
                           env=dict(os.environ, SPICEY_HIP_LIB=libpath), timeout=300)
        assert r.returncode == 0, r.stderr
        out = json.load(open(oj))
        assert "error" not in out, out
        t = out["ac"]
        assert t["freqs"] == g["freqs"] and t["keysV"] == g["keysV"] and t["keysI"] == g["keysI"]
        for k in g["keysV"]:
            assert cbits(cplx(t["V"][k]), cplx(g["V"][k])), (name, k)
        for k in g["keysI"]:
            assert cbits(cplx(t["I"][k]), cplx(g["I"][k])), (name, k)
