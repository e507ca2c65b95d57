"""The reference-order AC engine (spicey_ac_create with SpiceyOptions.interpreter = 3) on the CPU: the product's plan
(launch_plan.cpp), stamp lists (ac_exact_plan.cpp) and phase code (ac_exact_exec.h) run by tests/ac_exact_host/harness.cpp
with a serial executor, at 64 and 256 threads, in the LDS and the global layout, phases forwards and backwards, checked bit
for bit against the reference-generated goldens and the oracle (oracle/spicey_ref_ac.c)."""
import hashlib
import math
import os
import struct
import sys

import numpy as np
import pytest

from conftest import bits_equal, golden_netlist, load_golden
from spicey_amd import abi, ac as sac
from spicey_amd.netlist import parseNetlist
from test_oracle_ac import AC_SMALL, ac_golden_netlist, cbits, cplx

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "ac_exact_host"))
import pyacexact  # noqa: E402
from pyacexact import AcExactHostBackend, stamp_lists  # noqa: E402

LAYOUTS = [dict(T=64), dict(T=256), dict(T=64, global_ws=True), dict(T=256, global_ws=True, reverse=True)]
LAYOUT_IDS = ["T64", "T256", "T64_global", "T256_global_reverse"]
SKIP_GOLDENS = ["ac_skip_rc", "ac_skip_rl"]  # solveComplex.ts:46 drops a nonzero multiplier
# (golden, error class, message): "Complex divide by ~0" in elimination and at the last pivot; a sweep singular at its first
# frequency although an inductor refuses to divide at a later one (the default path's host check raises that one first)
ERROR_GOLDENS = [("ac_cdiv_elim", ZeroDivisionError, "Complex divide by ~0"), ("ac_cdiv_last", ZeroDivisionError, "Complex divide by ~0"),
                 ("ac_sing_first", sac.SingularComplexMatrixError, "Singular matrix (complex)"),
                 ("ac_err_float", sac.SingularComplexMatrixError, "Singular matrix (complex)")]


class Fixed:
    """Backend wrapper that substitutes the golden's phasors (the JS engine's cos / sin) for the host's."""

    def __init__(self, be, vph):
        self.be, self.vph = be, vph

    def run_ac(self, flat, freqs, vph, want_currents=True):
        return self.be.run_ac(flat, freqs, self.vph, want_currents)


def raw_same(a, b):
    """Status equal and, when it is 0, every bit of every voltage and current equal (the sign of zeros included)."""
    assert a["status"] == b["status"], (a.get("detail"), b.get("detail"))
    if a["status"] == 0:
        for k in ("out_v", "out_i"):
            x, y = np.asarray(a[k]), np.asarray(b[k])
            assert x.shape == y.shape and bits_equal(x.real, y.real).all() and bits_equal(x.imag, y.imag).all(), k


def check_golden_result(res, g):
    assert list(res["nodeVoltages"]) == g["keysV"] and list(res["elementCurrents"]) == g["keysI"]
    for k in g["keysV"]:
        assert cbits(res["nodeVoltages"][k], cplx(g["V"][k])), k
    for k in g["keysI"]:
        assert cbits(res["elementCurrents"][k], cplx(g["I"][k])), k
    assert sac.formatAcResult(res) == g["formatted"]


def sha_of(res, g):
    out = {}
    for key, series in (("sha256_V", res["nodeVoltages"]), ("sha256_I", res["elementCurrents"])):
        h = hashlib.sha256()
        for fi in range(len(g["freqs"])):
            for name in series:
                z = series[name][fi]
                h.update(struct.pack("<2d", z.real, z.imag))
        out[key] = h.hexdigest()
    return out


def first_failing_frequency(oracle_backend, flat, freqs, vph):
    """The frequency at which the reference throws (the oracle stops there): the first one that fails on its own."""
    for i in range(len(freqs)):
        if oracle_backend.run_ac(flat, np.asarray(freqs[i:i + 1]), vph)["status"] != 0:
            return i
    return -1


def random_ac_case(seed):
    """A random circuit of tests/random_circuits.py (AC ignores its diodes and switches) at random frequencies with random
    source phasors."""
    from random_circuits import random_netlist
    rng = np.random.default_rng(seed)
    flat = abi.flatten(parseNetlist(random_netlist(seed)))
    freqs = 10.0 ** rng.uniform(-1, 9, 3)
    vph = rng.normal(size=flat.nV) + 1j * rng.normal(size=flat.nV)
    return flat, freqs, vph


@pytest.mark.parametrize("layout", LAYOUTS, ids=LAYOUT_IDS)
@pytest.mark.parametrize("name", AC_SMALL + SKIP_GOLDENS)
def test_goldens_bit_exact(name, layout, oracle_backend):
    g = load_golden(name)
    ckt = parseNetlist(ac_golden_netlist(g))
    res = sac.simulateAC(ckt, backend=Fixed(AcExactHostBackend(**layout), cplx(g["vph"])), freqs=g["freqs"])
    check_golden_result(res, g)
    flat = abi.flatten(ckt)
    raw_same(AcExactHostBackend(**layout).run_ac(flat, np.array(g["freqs"]), cplx(g["vph"])), oracle_backend.run_ac(flat, np.array(g["freqs"]), cplx(g["vph"])))


@pytest.mark.parametrize("layout", [LAYOUTS[1], LAYOUTS[3]], ids=["T256", "T256_global_reverse"])
def test_large_golden_sha256(layout):
    g = load_golden("ac_rc1000")
    ckt = parseNetlist(ac_golden_netlist(g))
    res = sac.simulateAC(ckt, backend=Fixed(AcExactHostBackend(**layout), cplx(g["vph"])), freqs=g["freqs"])
    for k, v in g["V"].items():
        assert cbits(res["nodeVoltages"][k], cplx(v)), k
    for k, v in g["I"].items():
        assert cbits(res["elementCurrents"][k], cplx(v)), k
    assert sha_of(res, g) == {"sha256_V": g["sha256_V"], "sha256_I": g["sha256_I"]}


@pytest.mark.parametrize("name", SKIP_GOLDENS)
def test_skip_goldens_drop_multipliers(name):
    """The reference's |f| < EPS test drops nonzero multipliers here (the point of these goldens), at every frequency
    but the first of ac_skip_rc; node 3 then comes out as a signed zero, and its printed phase says which."""
    g = load_golden(name)
    flat = abi.flatten(parseNetlist(ac_golden_netlist(g)))
    for layout in LAYOUTS:
        res = AcExactHostBackend(**layout).run_ac(flat, np.array(g["freqs"]), cplx(g["vph"]))
        assert res["status"] == 0
        sk = res["skipped"][0]
        assert (sk[1:] > 0).all(), (name, sk)
        v3 = res["out_v"][0][1:, 2]
        assert (v3 == 0).all() and not np.signbit(v3.real).any() and not np.signbit(v3.imag).any()
    assert all(line.endswith(", 0.00000,0.00000") for line in g["formatted"].split("\n")[2:])


@pytest.mark.parametrize("name,exc,msg", ERROR_GOLDENS)
def test_error_goldens(name, exc, msg, oracle_backend):
    g = load_golden(name)
    assert g["error"] == msg
    ckt = parseNetlist(golden_netlist(g))
    for layout in LAYOUTS:
        with pytest.raises(exc, match=msg.replace("(", r"\(").replace(")", r"\)")):
            sac.simulateAC(ckt, backend=AcExactHostBackend(**layout))
    freqs = sac.buildFrequencyArray(**{k: g["acSpec"][k] for k in ("mode", "N", "f1", "f2")})
    flat, vph = abi.flatten(ckt), sac.source_phasors(ckt)
    res = AcExactHostBackend().run_ac(flat, np.array(freqs), vph)
    assert res["first"] == first_failing_frequency(oracle_backend, flat, freqs, vph)
    assert res["detail"] == f"{msg} at inst 0 frequency index {res['first']}"
    with pytest.raises(ValueError, match="R R1 must be > 0"):  # (a host check, before any solve)
        sac.simulateAC(parseNetlist(golden_netlist(load_golden("ac_err_r0"))), backend=AcExactHostBackend())


def test_first_failing_slot_is_instance_major():
    """Instance 0 fails at frequency index 2 (|wL|^2 < EPS at 1 Hz), instance 1 at index 0: the reference, run instance by
    instance, throws at (0, 2)."""
    text = "* divide\nV1 1 0 ac 1\nR1 1 2 1k\nL1 2 0 1n\n.ac lin 2 1 2\n.end\n"
    f0 = abi.flatten(parseNetlist(text))
    f1 = abi.flatten(parseNetlist(text.replace("1n", "1e-15")))
    flat = abi.stack_instances([f0, f1])
    res = AcExactHostBackend().run_ac(flat, np.array([1e6, 5e5, 1.0]), np.ones(1, np.complex128))
    assert res["status"] == abi.ERR_COMPLEX_DIV and res["first"] == 2
    assert res["slot_status"].tolist() == [[0, 0, 5], [5, 5, 5]]


@pytest.mark.parametrize("layout", [LAYOUTS[0], LAYOUTS[3]], ids=["T64", "T256_global_reverse"])
def test_random_circuits_against_oracle(layout, oracle_backend):
    n_err = 0
    for seed in range(200):
        flat, freqs, vph = random_ac_case(seed)
        ref = oracle_backend.run_ac(flat, freqs, vph)
        got = AcExactHostBackend(**layout).run_ac(flat, freqs, vph)
        raw_same(got, ref)
        if ref["status"] != 0:
            n_err += 1
            assert got["first"] == first_failing_frequency(oracle_backend, flat, freqs, vph), seed
    assert n_err < 100  # (diode-only nodes float in AC: some circuits are singular, most are not)


def test_series_rlc_resonance_against_oracle(oracle_backend):
    """At, next to and away from the L - C resonance (where the default path needs its dense fallback): bit for bit."""
    from random_circuits import series_rlc_ladder
    flats = [abi.flatten(parseNetlist(series_rlc_ladder(12, l=1e-3 * (1 + 0.25 * k)))) for k in range(4)]
    flat = abi.stack_instances(flats)
    f0 = 1.0 / (2.0 * math.pi * math.sqrt(1e-3 * 1e-6))
    freqs = np.array([f0 * (1.0 + d) for d in (1e-2, 1e-6, 1e-9, 1e-12, 0.0, -1e-10)] + [f0 / math.sqrt(1.25), 777.0])
    vph = np.ones(flat.nV, np.complex128)
    ref = oracle_backend.run_ac(flat, freqs, vph)
    assert ref["status"] == 0
    for layout in LAYOUTS:
        raw_same(AcExactHostBackend(**layout).run_ac(flat, freqs, vph), ref)


def _reference_lists(flat):
    """buildLinearSystemForAC replayed in Python: (row, column) -> [(kind, elem, which, sub)] in stamping order."""
    lists = {}
    nN, n = flat.n_nodes, flat.n_nodes + flat.nV

    def put(r, c, t):
        lists.setdefault((r, c), []).append(t)

    for kind, a, b, cnt in (("R", flat.R_n1, flat.R_n2, flat.nR), ("C", flat.C_n1, flat.C_n2, flat.nC), ("L", flat.L_n1, flat.L_n2, flat.nL)):
        for i in range(cnt):
            i1, i2 = int(a[i]) - 1, int(b[i]) - 1
            if i1 >= 0:
                put(i1, i1, (kind, i, 0, 0))
            if i2 >= 0:
                put(i2, i2, (kind, i, 0, 0))
            if i1 >= 0 and i2 >= 0:
                put(i1, i2, (kind, i, 0, 1))
                put(i2, i1, (kind, i, 0, 1))
    for k in range(flat.nV):
        i1, i2, j = int(flat.V_n1[k]) - 1, int(flat.V_n2[k]) - 1, nN + k
        one, mone = ("V", -1, 2, 0), ("V", -1, 2, 1)
        if i1 >= 0:
            put(i1, j, one)
        if i2 >= 0:
            put(i2, j, mone)
        if i1 >= 0:
            put(j, i1, one)
        if i2 >= 0:
            put(j, i2, mone)
        put(j, n, ("V", k, 0, 0))
    return sorted(lists.items())


@pytest.mark.parametrize("name", ["ac_rlc", "ac_two_src", "ac_mesh6", "ac_skip_rl"])
def test_stamp_lists_follow_the_reference(name):
    flat = abi.flatten(parseNetlist(ac_golden_netlist(load_golden(name))))
    assert stamp_lists(flat) == _reference_lists(flat)


def test_stamp_lists_of_shorted_elements():
    """An element with both terminals on one node adds twice and subtracts twice on one entry, in that order; a source
    from a node to itself adds and subtracts 1."""
    flat = abi.flatten(parseNetlist("* short\nV1 1 0 ac 1\nR1 1 2 1k\nR2 2 2 5\nC1 2 2 1u\nV2 2 2 ac 1\n.ac lin 2 1 2\n.end\n"))
    got = dict(stamp_lists(flat))
    assert got[(1, 1)] == [("R", 0, 0, 0), ("R", 1, 0, 0), ("R", 1, 0, 0), ("R", 1, 0, 1), ("R", 1, 0, 1), ("C", 0, 0, 0), ("C", 0, 0, 0),
                           ("C", 0, 0, 1), ("C", 0, 0, 1)]
    assert got[(1, 3)] == [("V", -1, 2, 0), ("V", -1, 2, 1)] and got[(3, 1)] == [("V", -1, 2, 0), ("V", -1, 2, 1)]
    assert stamp_lists(flat) == _reference_lists(flat)


def _ladder(n_nodes):
    from spicey_amd import synth
    return abi.flatten(parseNetlist(synth.rc_ladder(n=n_nodes, seed=1)))


def test_plan_threads_lds_and_chunks():
    small = abi.flatten(parseNetlist(ac_golden_netlist(load_golden("ac_rlc"))))
    p = pyacexact.plan(small)
    assert p["rc"] == 0 and p["threads"] == 64 and p["lds"] and p["lds_bytes"] == p["slot_bytes"]
    for T in (64, 128, 192, 256, 1024):
        assert pyacexact.plan(small, threads=T)["threads"] == T
    for T in (32, 65, 100, 1088, -64):
        bad = pyacexact.plan(small, threads=T)
        assert bad["rc"] == abi.ERR_BAD_DESC and "threads" in bad["error"]
    g = pyacexact.plan(small, force_global=True, slots=1000)
    assert not g["lds"] and g["lds_bytes"] == 0 and g["chunk"] == 1000
    # threads: 64 up to n = 64, 256 above; A | b in LDS while it fits 160 KiB (n up to about 97 on a ladder), else the slab
    sizes = {}
    for nodes in (62, 63, 64, 90, 96, 97, 98):
        f = _ladder(nodes)
        p = pyacexact.plan(f)
        n = p["n"]
        assert p["threads"] == (64 if n <= 64 else 256), n
        ld = (n + 1) | 1
        assert p["slot_bytes"] >= 16 * n * ld
        assert p["lds"] == (p["slot_bytes"] + 256 <= 160 * 1024), n
        sizes[n] = p["lds"]
    assert sizes[max(k for k, v in sizes.items() if v)] and not sizes[max(sizes)] and 95 <= max(k for k, v in sizes.items() if v) <= 99
    # the global slab of one launch stays within 1 GiB: rc_ladder(1000) slots are ~16 MB
    big = pyacexact.plan(_ladder(1000), slots=500)
    assert not big["lds"] and big["threads"] == 256
    assert big["chunk"] == (1 << 30) // big["slot_bytes"] and big["chunk"] * big["slot_bytes"] <= (1 << 30)


def v8_hypot(x, y):
    """V8's Math.hypot(x, y), restated elementwise in numpy (IEEE double, no contraction, correctly rounded sqrt)."""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    ax, ay = np.abs(x), np.abs(y)
    mx = np.maximum(np.where(np.isnan(ax), 0.0, ax), np.where(np.isnan(ay), 0.0, ay))
    with np.errstate(all="ignore"):
        a0, a1 = ax / mx, ay / mx
        s0 = a0 * a0 - 0.0
        p0 = 0.0 + s0
        comp = (p0 - 0.0) - s0
        s1 = a1 * a1 - comp
        out = np.sqrt(p0 + s1) * mx
    nan = np.isnan(x) | np.isnan(y)
    out = np.where(mx == 0.0, 0.0, out)
    out = np.where(nan, np.nan, out)
    return np.where(np.isinf(x) | np.isinf(y), np.inf, out)


def hypot_cases(n, seed=5):
    """Pairs that stress the algorithm: near-ties, one tiny against one large, zeros of both signs, subnormals, huge
    values, Inf and NaN."""
    rng = np.random.default_rng(seed)
    m = n // 6
    a = rng.normal(size=m) * 10.0 ** rng.integers(-300, 300, m)
    parts = [np.stack([a, a * (1 + rng.integers(-8, 8, m) * 2.0 ** -52)], 1),                                 # near-ties
             np.stack([rng.normal(size=m), rng.normal(size=m) * 10.0 ** rng.uniform(-20, 0, m)], 1),       # ordinary / small
             np.stack([rng.normal(size=m) * 1e-310, rng.normal(size=m) * 1e-315], 1),                      # subnormals
             np.stack([rng.normal(size=m) * 1e307, rng.normal(size=m) * 1e307], 1),                        # overflow of the squares
             np.stack([rng.normal(size=m), rng.choice([0.0, -0.0, 5e-324, -5e-324], m)], 1),               # zeros, the smallest
             np.stack([rng.choice([np.inf, -np.inf, np.nan, 0.0, -0.0, 1.0], n - 5 * m), rng.choice([np.inf, -np.inf, np.nan, 0.0, 2.0], n - 5 * m)], 1)]
    xy = np.concatenate(parts)
    return xy[:, 0].copy(), xy[:, 1].copy()


def test_hypot_is_v8s():
    x, y = hypot_cases(120000)
    got, want = pyacexact.hypot(x, y), v8_hypot(x, y)
    assert bits_equal(got, want).all()
    assert np.isinf(pyacexact.hypot([np.nan, np.inf], [np.inf, np.nan])).all() and np.isnan(pyacexact.hypot([np.nan], [1.0])).all()
    assert pyacexact.hypot([3.0], [4.0])[0] == 5.0


def test_default_path_host_checks_unchanged():
    """Without exact_order the inductor's divide error is still the host's, raised before any solve (no backend runs)."""

    class Never:
        def run_ac(self, *a, **k):
            raise AssertionError("no solve expected")

    with pytest.raises(ZeroDivisionError):
        sac.simulateAC(parseNetlist(golden_netlist(load_golden("ac_sing_first"))), backend=Never())
    with pytest.raises(ValueError):
        sac.simulateAC(parseNetlist(golden_netlist(load_golden("ac_skip_rc"))), backend=Never(), exact_order=True)
