"""AC sensitivity analysis on the CPU: the formulas against the unchanged oracle by central differences, closed forms, the
impedance-scaling rule, the reduction of sens_exec.h bit for bit against reduce_reference_sens, and the interface of
simulateSens / simulateSensBatch with the harness (tests/sens_host) behind the backend interface.

Bars.  Central differences: per (frequency, element) |S - FD_h| <= |FD_2h - FD_h| + (1e-9 |H| + 1e-12) / h with h = 1e-3 — the
first term is three times the Richardson estimate of FD_h's truncation error, the second the project's parity bar
(ac_resident_cases.py) on the two oracle runs carried through the quotient — on frequencies at which the largest bar is at
most 1e-3 of max_e |S_e|, so that a wrong sign or a lost factor cannot hide.  Closed forms: 3e-9 |ref| + 1e-12, three factors
(two currents and H) each at the project's bar.  Scaling rule: 1e-9 sum_e |S_e|."""
import math

import numpy as np
import pytest

from batch_variants import variant
from conftest import golden_netlist, load_golden
from spicey_amd import abi
from spicey_amd.ac import SingularComplexMatrixError
from spicey_amd.ac_batch import source_phasors
from spicey_amd.netlist import parseNetlist
from spicey_amd.sens import reduce_reference_sens, simulateSens, simulateSensBatch

from sens_host import pysens as ps

H_STEP = 1e-3
TWO_STAGE = "V1 in 0 AC 1\nR1 in a 1000\nC1 a 0 1e-9\nR2 a out 2200\nC2 out 0 4.7e-10\nR3 out 0 1e5\n.ac dec 5 1e3 1e7\n.end\n"


def _ac_lines(text):
    """The netlist without diodes, switches and models (simulateAC stamps R, C, L, V)."""
    return "\n".join(ln for ln in text.split("\n") if ln[:1].upper() not in ("D", "S") and not ln.lower().startswith(".model"))


def _rlc_ladder_text():
    from random_circuits import series_rlc_ladder
    return series_rlc_ladder(3, r=100.0)  # Q = sqrt(L / C) / R = 0.32


def _random_text():
    """random_netlist(13) — 7 R, 4 C, 2 L — with an AC phasor on its source (the generator's sources have none)."""
    from random_circuits import random_netlist
    lines = _ac_lines(random_netlist(13)).split("\n")
    return "\n".join(" ".join(ln.split()[:3]) + " AC 1" if ln[:1] == "V" else ln for ln in lines)


# (name, netlist, output, frequencies: four per circuit, away from sharp resonances)
FD_CASES = [
    ("two_stage_rc", lambda: TWO_STAGE, "v(out)", (1e3, 4e4, 3e5, 5e6)),
    ("rlc_ladder", _rlc_ladder_text, "v(b2)", (300.0, 2e3, 7e3, 4e4)),
    ("random13", _random_text, "v(n1)", (1e2, 1e4, 1e6, 1e8)),
]


def _fd_case(name, text_of, output, freqs):
    ckt = parseNetlist(text_of())
    return ckt, output, np.asarray(freqs, dtype=np.float64)


_FD_CACHE = {}


def _oracle_fd(name, ckt, output, freqs, oracle_backend):
    """(H [nf], FD_h [nf][nE], FD_2h [nf][nE]) of the oracle: p_e d out / d p_e by central differences of relative step h and
    2h, one oracle sweep per perturbed value.  Computed once per circuit."""
    if name in _FD_CACHE:
        return _FD_CACHE[name]
    node = ckt.nodes.get(output[2:-1])
    flat = abi.flatten(ckt)
    vph = source_phasors(ckt)

    def out_of():
        r = oracle_backend.run_ac(flat, freqs, vph)
        assert r["status"] == 0
        return np.array(r["out_v"][0][:, node - 1])

    H = out_of()
    cols = [(flat.R_val, i) for i in range(flat.nR)] + [(flat.C_val, i) for i in range(flat.nC)] + [(flat.L_val, i) for i in range(flat.nL)]
    fd = {}
    for h in (H_STEP, 2 * H_STEP):
        rows = []
        for arr, i in cols:
            p = arr[0, i]
            arr[0, i] = p * (1 + h)
            up = out_of()
            arr[0, i] = p * (1 - h)
            dn = out_of()
            arr[0, i] = p
            rows.append((up - dn) / (2 * h))
        fd[h] = np.stack(rows, axis=1)
    _FD_CACHE[name] = (H, fd[H_STEP], fd[2 * H_STEP])
    return _FD_CACHE[name]


def _host_S(ckt, output, freqs, resident):
    """(H [nf], S [nf][nE]) of the code under test: S_e = (m_e + j phi_e) H from the full result of the host backend."""
    r = simulateSens(ckt, output, freqs=freqs, full=True, backend=ps.HostSensBackend(resident=resident))
    H = np.array(r["h"])
    names = [e.name for e in ckt.R] + [e.name for e in ckt.C] + [e.name for e in ckt.L]
    rel = np.stack([np.array(r["mag_sens"][n]) + 1j * np.radians(np.array(r["phase_sens_deg"][n])) for n in names], axis=1)
    return H, rel * H[:, None], (len(ckt.R), len(ckt.C), len(ckt.L))


@pytest.mark.parametrize("case", FD_CASES, ids=[c[0] for c in FD_CASES])
@pytest.mark.parametrize("resident", (False, True), ids=("per_solve", "resident"))
def test_sensitivities_against_central_differences_of_the_oracle(case, resident, oracle_backend):
    ckt, output, freqs = _fd_case(*case)
    H, fd1, fd2 = _oracle_fd(case[0], ckt, output, freqs, oracle_backend)
    bar = np.abs(fd2 - fd1) + (1e-9 * np.abs(H)[:, None] + 1e-12) / H_STEP
    # the condition, on the oracle alone: the bar resolves the largest sensitivity to 1e-3 at every frequency
    assert (bar.max(axis=1) <= 1e-3 * np.abs(fd1).max(axis=1)).all(), (case[0], bar.max(axis=1) / np.abs(fd1).max(axis=1))
    Hh, S, _ = _host_S(ckt, output, freqs, resident)
    assert (np.abs(Hh - H) <= 1e-9 * np.abs(H) + 1e-12).all()
    ratio = np.abs(S - fd1) / bar
    print(f"{case[0]} ({'resident' if resident else 'per-solve'}): worst error {ratio.max():.3g} of the bar, largest bar "
          f"{(bar.max(axis=1) / np.abs(fd1).max(axis=1)).max():.3g} of max |S|")
    assert (ratio <= 1.0).all(), (case[0], ratio.max())


@pytest.mark.parametrize("case", FD_CASES, ids=[c[0] for c in FD_CASES])
def test_impedance_scaling_rule(case):
    """Scaling every impedance by one factor (R and L up, C down) leaves a voltage ratio unchanged: sum_R S - sum_C S + sum_L S
    = 0 at every frequency."""
    ckt, output, freqs = _fd_case(*case)
    for resident in (False, True):
        _, S, (nR, nC, nL) = _host_S(ckt, output, freqs, resident)
        rule = S[:, :nR].sum(axis=1) - S[:, nR:nR + nC].sum(axis=1) + S[:, nR + nC:].sum(axis=1)
        scale = np.abs(S).sum(axis=1)
        print(f"{case[0]}: scaling rule {np.max(np.abs(rule) / scale):.3g} of sum |S|")
        assert (scale > 0).all() and (np.abs(rule) <= 1e-9 * scale).all(), (case[0], np.abs(rule) / scale)


# ---- closed forms --------------------------------------------------------------------------------------------------------
def _rel(r, name):
    return np.array(r["mag_sens"][name]) + 1j * np.radians(np.array(r["phase_sens_deg"][name]))


def _close(got, ref):
    return (np.abs(got - ref) <= 3e-9 * np.abs(ref) + 1e-12).all()


@pytest.mark.parametrize("resident", (False, True), ids=("per_solve", "resident"))
def test_divider_closed_form(resident):
    ckt = parseNetlist("V1 in 0 AC 1\nR1 in out 3000\nR2 out 0 1000\n.ac dec 2 10 1e4\n.end\n")
    r = simulateSens(ckt, "v(out)", full=True, backend=ps.HostSensBackend(resident=resident))
    n = len(r["freqs"])
    assert _close(_rel(r, "R1"), np.full(n, -0.75 + 0j)) and _close(_rel(r, "R2"), np.full(n, 0.75 + 0j))
    assert _close(np.array(r["h"]), np.full(n, 0.25 + 0j))
    # tol = None is 1.0 per element: the worst case is |m_R1| + |m_R2|, the sigma their root sum square
    assert _close(np.array(r["mag_wc"]), np.full(n, 1.5)) and _close(np.array(r["mag_sigma"]), np.full(n, 0.75 * math.sqrt(2)))
    assert _close(np.array(r["phase_wc_deg"]), np.zeros(n)) and _close(np.array(r["mag_wc_db"]), np.full(n, 20 * math.log10(2.5)))
    e = r["elements"]
    assert set(e) == {"R1", "R2"} and e["R1"]["kind"] == "R" and e["R1"]["value"] == 3000.0 and e["R2"]["tol"] == 1.0
    assert abs(e["R1"]["mag_peak"] + 0.75) <= 3e-9 and abs(e["R2"]["mag_peak"] - 0.75) <= 3e-9
    # across R1: H = R1 / (R1 + R2), the signs swap and the magnitude is R2 / (R1 + R2)
    d = simulateSens(ckt, "v(in,out)", full=True, backend=ps.HostSensBackend(resident=resident))
    assert _close(_rel(d, "R1"), np.full(n, 0.25 + 0j)) and _close(_rel(d, "R2"), np.full(n, -0.25 + 0j))


@pytest.mark.parametrize("resident", (False, True), ids=("per_solve", "resident"))
def test_rc_low_pass_closed_form(resident):
    """H = 1 / (1 + jwRC): S_R / H = S_C / H = -jwRC / (1 + jwRC)."""
    ckt = parseNetlist("V1 in 0 AC 1\nR1 in out 1000\nC1 out 0 1e-9\n.ac dec 5 1e3 1e7\n.end\n")
    r = simulateSens(ckt, "v(out)", tol={"R1": 0.01, "C": 0.05}, full=True, backend=ps.HostSensBackend(resident=resident))
    w = 2 * np.pi * np.array(r["freqs"])
    ref = -1j * w * 1e-6 / (1 + 1j * w * 1e-6)
    assert _close(_rel(r, "R1"), ref) and _close(_rel(r, "C1"), ref)
    assert _close(np.array(r["h"]), 1 / (1 + 1j * w * 1e-6))
    assert _close(np.array(r["mag_wc"]), 0.06 * np.abs(ref.real)) and _close(np.array(r["mag_sigma"]), math.hypot(0.01, 0.05) * np.abs(ref.real))
    assert _close(np.array(r["phase_wc_deg"]), np.degrees(0.06 * np.abs(ref.imag)))
    # |m| grows with w towards 1, |phi| peaks at w RC = 1 (f = 159 kHz: the listed 1.58e5); C1 (5 %) ranks before R1 (1 %)
    e = r["elements"]
    assert list(e) == ["C1", "R1"] and e["C1"]["f_mag_peak"] == r["freqs"][-1] and abs(e["C1"]["f_phase_peak"] - 1.585e5) < 1e3
    assert abs(e["R1"]["phase_peak_deg"] + math.degrees(0.5)) < 0.01


@pytest.mark.parametrize("resident", (False, True), ids=("per_solve", "resident"))
def test_series_rlc_closed_form_at_and_off_resonance(resident):
    """Series R - L - C read across C: H = 1 / D with D = 1 - w^2 LC + jwRC; S_R / H = -jwRC / D, S_L / H = w^2 LC / D, S_C / H =
    (w^2 LC - jwRC) / D.  At w0 (Q = 3.16, where the static pivot order of the sweep meets its cancelling diagonal) and off it."""
    Rv, Lv, Cv = 10.0, 1e-3, 1e-6
    f0 = 1.0 / (2 * math.pi * math.sqrt(Lv * Cv))
    freqs = np.array([0.2 * f0, 0.9 * f0, f0, 1.3 * f0, 6 * f0])
    ckt = parseNetlist(f"V1 in 0 AC 1\nR1 in a {Rv}\nL1 a b {Lv}\nC1 b 0 {Cv}\n.end\n")
    r = simulateSens(ckt, "v(b)", freqs=freqs, full=True, backend=ps.HostSensBackend(resident=resident))
    w = 2 * np.pi * freqs
    D = 1 - w * w * Lv * Cv + 1j * w * Rv * Cv
    assert _close(np.array(r["h"]), 1 / D)
    assert _close(_rel(r, "R1"), -1j * w * Rv * Cv / D)
    assert _close(_rel(r, "L1"), w * w * Lv * Cv / D)
    assert _close(_rel(r, "C1"), (w * w * Lv * Cv - 1j * w * Rv * Cv) / D)


# ---- the reduction ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ps.REDUCTION_SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("nf", ps.REDUCTION_NF)
def test_reduction_is_the_reference_bit_for_bit(shape, nf):
    """Three instances with values of their own; the whole sweep, one frequency and the last two; the three forms of the output
    pair; the first frequency 0 (the capacitors' q == 0 rows); H = 0 in one slot (inf / NaN, the same bits); tolerances with
    zeros; with and without d_full, d_peak the same both ways."""
    nR, nC, nL = shape
    nE = nR + nC + nL
    out_v, i_dir, i_adj, R, Cv, Lv, tol, freqs = ps.sens_inputs(3, nf, shape, 3, 3, seed=1000 * nE + nf)
    freqs[0] = 0.0
    out_v[1, nf // 2, :] = 0.0
    for (k0, k1) in ps.windows(nf):
        for (op, on) in ps.REDUCTION_PAIRS:
            req = abi.ac_sens_req(op, on, nR, nC, nL, k0, k1)
            with np.errstate(all="ignore"):
                spec, peak, full = ps.reduce(out_v, i_dir, i_adj, R, Cv, Lv, tol, freqs, req, full=True)
                spec0, peak0, none = ps.reduce(out_v, i_dir, i_adj, R, Cv, Lv, tol, freqs, req, full=False)
            ref = reduce_reference_sens(out_v, i_dir, i_adj, R, Cv, Lv, tol, freqs, op, on, k0, k1)
            for g, r, what in zip((spec, peak, full), ref, ("spec", "peak", "full")):
                assert g.shape == r.shape and ps.bits_equal(g, r).all(), (what, shape, nf, k0, k1, op, on)
            assert none is None and ps.bits_equal(spec0, spec).all() and ps.bits_equal(peak0, peak).all()
            # the capacitors' rows at f = 0 are zero, the slot with H = 0 is not finite, every other slot is
            assert (full[[0, 2], 0, nR:nR + nC] == 0).all()
            finite = np.isfinite(full).all(axis=(2, 3))
            assert not finite[1, nf // 2] and finite.sum() == 3 * nf - 1
            assert not np.isfinite(spec[1, nf // 2, 2:]).any() and (spec[finite][:, 2:] >= 0).all()
            # a peak is a row of d_full inside the window, and no row of the window is larger
            kk1 = nf - 1 if k1 == -1 else k1
            for col in (0, 2):
                at = peak[:, :, col + 1].astype(int)
                assert (at >= k0).all() and (at <= kk1).all()
                val = np.take_along_axis(full[:, :, :, col // 2], at[:, None, :], axis=1)[:, 0, :]
                assert ps.bits_equal(val, peak[:, :, col]).all()
                ok = np.isfinite(full[:, k0:kk1 + 1, :, col // 2]).all(axis=1)
                assert (np.abs(full[:, k0:kk1 + 1, :, col // 2]).max(axis=1)[ok] == np.abs(peak[:, :, col])[ok]).all()


def test_reduction_refusals():
    shape = (4, 2, 1)
    out_v, i_dir, i_adj, R, Cv, Lv, tol, freqs = ps.sens_inputs(2, 5, shape, 2, 2, seed=7)
    ok = dict(out_p=0, out_n=-1, nR=4, nC=2, nL=1, k_from=0, k_to=-1)

    def refused(text, call=None, tl=None, **kw):
        req = abi.ac_sens_req(**{**ok, **{k: v for k, v in kw.items() if k in ok}})
        for k, v in kw.items():
            if k in ("reserved", "struct_bytes"):
                setattr(req, k, v)
        with pytest.raises(ps.Refused, match=text) as e:
            ps.reduce(out_v, i_dir, i_adj, R, Cv, Lv, tol if tl is None else tl, freqs, req, **(call or {}))
        assert "sens" in str(e.value)

    ps.reduce(out_v, i_dir, i_adj, R, Cv, Lv, tol, freqs, abi.ac_sens_req(**ok))
    refused("column out of range", out_p=2)
    refused("column out of range", out_n=-2)
    refused("one node twice", out_p=1, out_n=1)
    refused("one node twice", out_p=-1, out_n=-1)
    refused("window", k_from=3, k_to=2)
    refused("window", k_to=5)
    refused("window", k_from=-1)
    refused("reserved", reserved=1)
    refused("struct_bytes", struct_bytes=40)
    refused("null buffer", call=dict(have_out=False))
    refused("null buffer", call=dict(have_tol=False))
    refused("workspace", call=dict(work_bytes=8))
    refused("bad counts", call=dict(n_inst=0))
    refused("bad counts", call=dict(n_freq=0))
    refused("bad counts", nC=-1)
    refused("no element", nR=0, nC=0, nL=0)
    refused("exceeds", nL=4)
    for bad in (-1e-3, math.nan, math.inf):
        t = tol.copy()
        t[-1] = bad
        refused("tolerance", tl=t)
    # (a kind whose count is 0 needs no buffer; one whose count is not does)
    with pytest.raises(ps.Refused, match="null buffer"):
        ps.reduce(out_v, i_dir, i_adj, R, np.zeros((2, 0)), Lv, tol, freqs, abi.ac_sens_req(**ok))
    assert ps.lib().spicey_sens_host_workspace_bytes(0, 5, 7) == -1 and ps.lib().spicey_sens_host_workspace_bytes(2, 5, 0) == -1


# ---- the interface -------------------------------------------------------------------------------------------------------
RC = "V1 in 0 AC 1\nR1 in out 1000\nC1 out 0 1e-9\n.ac dec 5 1e3 1e7\n.end\n"


def test_request_and_tolerance_refusals():
    ckt = parseNetlist(RC)
    be = ps.HostSensBackend()
    with pytest.raises(ValueError, match="no node named"):
        simulateSens(ckt, "v(nowhere)", backend=be)
    with pytest.raises(ValueError, match="one node twice"):
        simulateSens(ckt, "v(out,out)", backend=be)
    with pytest.raises(ValueError, match="v\\(node\\)"):
        simulateSens(ckt, "i(R1)", backend=be)
    with pytest.raises(ValueError, match="window is empty"):
        simulateSens(ckt, "v(out)", f_from=1e9, backend=be)
    with pytest.raises(ValueError, match="neither an R, C or L"):
        simulateSens(ckt, "v(out)", tol={"R7": 0.01}, backend=be)
    with pytest.raises(ValueError, match="neither an R, C or L"):
        simulateSens(ckt, "v(out)", tol={"V1": 0.01}, backend=be)
    for bad in (-0.01, math.nan, math.inf, "1%"):
        with pytest.raises(ValueError, match="tolerance"):
            simulateSens(ckt, "v(out)", tol=bad, backend=be)
        with pytest.raises(ValueError, match="tolerance"):
            simulateSens(ckt, "v(out)", tol={"r1": bad}, backend=be)
        with pytest.raises(ValueError, match="tolerance"):
            simulateSens(ckt, "v(out)", tol={"C": bad}, backend=be)
    with pytest.raises(ValueError, match="share the name"):
        simulateSens(parseNetlist("V1 in 0 AC 1\nR1 in out 1k\nR1 out 0 1k\n.ac dec 2 10 1e3\n.end\n"), "v(out)", backend=be)
    with pytest.raises(ValueError, match="no R, C or L"):
        simulateSens(parseNetlist("V1 in 0 AC 1\n.ac dec 2 10 1e3\n.end\n"), "v(in)", backend=be)
    with pytest.raises(ValueError, match="exact_order"):  # the reference-order engine (interpreter = 3) has no injection
        simulateSens(ckt, "v(out)", exact_order=True)
    with pytest.raises(TypeError, match="run_ac_sens"):
        simulateSens(ckt, "v(out)", backend=object())
    assert be.launches == []  # a refused request runs nothing
    nocard = parseNetlist("V1 in 0 AC 1\nR1 in out 1k\nC1 out 0 1n\n.end\n")
    assert simulateSens(nocard, "v(out)", backend=be) is None
    got = simulateSens(nocard, "v(out)", tol={"r1": 0.01, "C": 0.1, "R": 0.5}, freqs=[1e3, 1e4], f_from=5e3, backend=be)
    assert got["freqs"] == [1e3, 1e4] and be.launches == [1] and got["band"] == (1e4, 1e4)
    assert got["elements"]["R1"]["tol"] == 0.01 and got["elements"]["C1"]["tol"] == 0.1 and "mag_sens" not in got
    assert got["elements"]["R1"]["f_mag_peak"] == 1e4
    assert simulateSens(nocard, "v(out)", tol={"C": 0.1}, freqs=[1e3], backend=be)["elements"]["R1"]["tol"] == 0.0


def _same(one, other, where):
    assert list(one) == list(other)
    for k in one:
        a, b = one[k], other[k]
        if k == "elements":
            assert list(a) == list(b), (where, k)
            for n in a:
                assert list(a[n].values()) == list(b[n].values()), (where, n)
        elif isinstance(a, dict):
            assert list(a) == list(b) and all(np.asarray(a[n]).tobytes() == np.asarray(b[n]).tobytes() for n in a), (where, k)
        else:
            assert np.asarray(a).tobytes() == np.asarray(b).tobytes(), (where, k)


def test_batch_groups_by_topology_and_equals_single_calls():
    """Variants of two topologies, interleaved, with one circuit without a card: one launch per topology, each slot what
    simulateSens gives for that circuit alone (bit for bit: the host sweep does not depend on the batch)."""
    nocard = "V1 in 0 AC 1\nR1 in out 1k\nC1 out 0 1n\n.end\n"
    texts = [variant(RC, 0), variant(TWO_STAGE, 0), nocard, variant(RC, 1), variant(TWO_STAGE, 2), variant(RC, 3)]
    ckts = [parseNetlist(t) for t in texts]
    be = ps.HostSensBackend()
    kw = dict(tol={"R": 0.01, "C": 0.05}, f_from=1e4, f_to=1e6, full=True)
    res = simulateSensBatch(ckts, "v(out)", backend=be, **kw)
    assert be.launches == [3, 2] and res[2] is None
    for i, c in enumerate(ckts):
        if i == 2:
            continue
        one = simulateSens(c, "v(out)", backend=ps.HostSensBackend(), **kw)
        _same(one, res[i], i)
        assert one["band"] == (1e4, 1e6)
    split = ps.HostSensBackend()
    simulateSensBatch(ckts, "v(out)", backend=split, max_instances=2)
    assert split.launches == [2, 1, 2]
    # `full` counts in max_result_bytes: n_freq x 2 elements x 16 bytes more per instance
    small = ps.HostSensBackend()
    rc3 = [ckts[0], ckts[3], ckts[5]]
    nf = len(res[0]["freqs"])
    per = nf * abi.SENS_SPEC * 8 + 2 * abi.SENS_PEAK * 8
    per_full = per + nf * 2 * 16
    assert 3 * per <= 2 * per_full < 3 * per_full
    simulateSensBatch(rc3, "v(out)", backend=small, max_result_bytes=2 * per_full)
    simulateSensBatch(rc3, "v(out)", backend=small, max_result_bytes=2 * per_full, full=True)
    assert small.launches == [3, 2, 1]


def test_a_singular_instance_in_its_slot():
    """ac_sing_first among variants of its benign form: its slot holds the error simulateAC raises, the others their
    results."""
    sing = golden_netlist(load_golden("ac_sing_first"))
    benign = sing.replace("L1 2 3 1e-18", "L1 2 3 1m")
    texts = [variant(benign, 1), sing, variant(benign, 2)]
    res = simulateSensBatch([parseNetlist(t) for t in texts], "v(2)", tol=0.01, backend=ps.HostSensBackend())
    assert isinstance(res[1], SingularComplexMatrixError)
    for k in (0, 2):
        assert isinstance(res[k], dict) and np.isfinite(res[k]["mag_wc"]).all() and max(res[k]["mag_wc"]) > 0
    with pytest.raises(SingularComplexMatrixError):
        simulateSens(parseNetlist(sing), "v(2)", backend=ps.HostSensBackend())


def test_a_failure_of_the_injected_sweep_alone_reaches_its_instance(monkeypatch):
    """Status merging: a slot's word is D's where nonzero, else X's.  The matrix of both sweeps is the same, so a solve that
    fails in X alone does not come about by itself: the injected sweep's table is marked by hand."""
    ckts = [parseNetlist(variant(RC, k)) for k in range(3)]
    real = ps.sweep

    def marked(flat, freqs, vph, node_p=0, node_n=0, amp=1.0, **kw):
        r = real(flat, freqs, vph, node_p, node_n, amp, **kw)
        if vph is None:  # sweep X
            r["slot_status"][1, 4] = 2
            r["slot_status"][1, 9] = 1
        else:
            r["slot_status"][2, 7] = 1
        return r

    monkeypatch.setattr(ps, "sweep", marked)
    be = ps.HostSensBackend()
    res = simulateSensBatch(ckts, "v(out)", backend=be)
    assert be.launches == [3] and isinstance(res[0], dict)
    assert isinstance(res[1], ZeroDivisionError) and isinstance(res[2], SingularComplexMatrixError)
    d = {"slot_status": np.array([[0, 1, 0], [0, 0, 0]])}
    x = {"slot_status": np.array([[2, 0, 0], [0, 0, 2]])}
    rc, inst, first, _ = ps.merged_status(d, x)
    assert rc == abi.ERR_COMPLEX_DIV and inst.tolist() == [abi.ERR_COMPLEX_DIV, abi.ERR_COMPLEX_DIV] and first.tolist() == [0, 2]
