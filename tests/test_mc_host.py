"""Monte Carlo tolerance analysis on the CPU: the draw's statistics, Philox's known answers, the draw and the reduction of
mc_exec.h bit for bit against the numpy definitions of spicey_amd.mc, every refusal of the two judges, the reduction of the
unchanged oracle's sweeps, and simulateMonteCarlo with the harness (tests/mc_host) behind the backend interface.

Bars.  Draw statistics (seed 1, n = 4096): a sample mean within 5 standard errors of the table's mean, a sample standard deviation
within 10 % of the table's (its own standard error at n = 4096 is about 1 % for a uniform and 1.1 % for a truncated Gaussian
deviate).  The table's mean and variance are those of the piecewise-linear inverse distribution function the draw interpolates:
per interval of ends a, b the mean (a + b) / 2 and the second moment (a a + a b + b b) / 3.  Closed form: 3e-9 |ref| + 1e-12, the
bar of test_sens_host.py; an order statistic is 1-Lipschitz in the sup norm of the samples, so the bar carries over."""
import math

import numpy as np
import pytest

from conftest import golden_netlist, load_golden
from spicey_amd import abi
from spicey_amd.ac_batch import source_phasors
from spicey_amd.mc import (draw_reference_mc, icdf_table, mc_deviates, mc_ranks, mc_uniform, mc_values, philox4x32, quantile_curves, reduce_reference_mc,
                           simulateMonteCarlo)
from spicey_amd.netlist import parseNetlist

from mc_host import pymc as pm
from sens_host import pysens as ps

KAT = (((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
       ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
       ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)))
RC = "V1 in 0 AC 1\nR1 in out 1000\nC1 out 0 1e-9\n.ac dec 5 1e3 1e7\n.end\n"


def _table_moments(icdf):
    a, b = icdf[:-1], icdf[1:]
    mean = ((a + b) / 2).mean()
    second = ((a * a + a * b + b * b) / 3).mean()
    return mean, math.sqrt(second - mean * mean)


# ---- the draw -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dist", ("uniform", "gauss"))
def test_draw_statistics(dist):
    """Seed 1, n = 4096, 8 elements: deterministic, on the numpy draw whose bits the tests below tie to the harness."""
    n, nE = 4096, 8
    icdf, log2K = icdf_table(dist)
    m = mc_uniform(1, n, nE)
    assert m.dtype == np.uint64 and int(m.max()) < 1 << 52 and len(np.unique(m)) == n * nE
    assert (pm.uniform(1, n, nE) == m).all()
    d = mc_deviates(m, icdf, log2K)
    assert (np.abs(d) <= 1.0).all()
    mean, sd = _table_moments(icdf)
    for e in range(nE):
        assert abs(d[:, e].mean() - mean) <= 5 * sd / math.sqrt(n), (dist, e, d[:, e].mean())
        assert abs(d[:, e].std(ddof=1) - sd) <= 0.1 * sd, (dist, e, d[:, e].std(ddof=1), sd)
    if dist == "gauss":  # tol is 3 sigma, truncated: the deviate's sigma is a little under 1 / 3
        assert 0.32 < sd < 1 / 3


def test_philox_known_answers():
    for counter, key, want in KAT:
        assert pm.philox(counter, key).tolist() == list(want)
        assert philox4x32(np.array(counter, np.uint64), key).tolist() == list(want)
    assert philox4x32(np.array([k[0] for k in KAT[:1]] * 3, np.uint64), KAT[0][1]).shape == (3, 4)


@pytest.mark.parametrize("shape", ps.REDUCTION_SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("ni", pm.DRAW_NI)
@pytest.mark.parametrize("log2K", pm.DRAW_L)
def test_draw_is_the_reference_bit_for_bit(shape, ni, log2K):
    nE = sum(shape)
    R, Cv, Lv, tol, icdf = pm.draw_inputs(ni, shape, log2K, seed=100 * nE + 10 * ni + log2K)
    seed = 0x9E3779B97F4A7C15 ^ (nE << 33) ^ ni
    for keep in (False, True):
        got = pm.draw(R, Cv, Lv, tol, icdf, abi.ac_mc_req(0, -1, log2K, keep, seed))
        ref = draw_reference_mc(R, Cv, Lv, tol, icdf, log2K, seed, keep)
        for g, r, nom, what in zip(got, ref, (R, Cv, Lv), "RCL"):
            assert g.shape == r.shape and pm.bits_equal(g, r).all(), (what, shape, ni, log2K, keep)
            assert (g > 0).all() and np.isfinite(g).all()
        # a zero tolerance leaves its element nominal in every sample
        nR, nC, _ = shape
        zero = tol == 0
        assert zero.any()
        assert pm.bits_equal(got[0][:, zero[:nR]], (1.0 / R)[:, zero[:nR]]).all()
        assert pm.bits_equal(got[1][:, zero[nR:nR + nC]], Cv[:, zero[nR:nR + nC]]).all()
        assert pm.bits_equal(got[2][:, zero[nR + nC:]], Lv[:, zero[nR + nC:]]).all()
        if keep:  # sample 0 is the nominal bits; its 1 / R is the quotient 1.0 / R
            assert pm.bits_equal(got[0][0], 1.0 / R[0]).all() and pm.bits_equal(got[1][0], Cv[0]).all() and pm.bits_equal(got[2][0], Lv[0]).all()
        elif nE > 3:
            assert not pm.bits_equal(np.concatenate([g[0] for g in got]), np.concatenate([(1.0 / R)[0], Cv[0], Lv[0]])).all()
    # another seed gives other values
    other = pm.draw(R, Cv, Lv, tol, icdf, abi.ac_mc_req(0, -1, log2K, False, seed + 1))
    if nE > 3:
        assert not all(pm.bits_equal(a, b).all() for a, b in zip(other, got))


def test_draw_refusals():
    shape = (4, 2, 1)
    R, Cv, Lv, tol, icdf = pm.draw_inputs(3, shape, 3, seed=7)

    def refused(text, tl=tol, tab=icdf, call=None, **kw):
        req = abi.ac_mc_req(0, -1, kw.pop("log2K", 3), True, 5)
        for k, v in kw.items():
            setattr(req, k, v)
        with pytest.raises(pm.Refused, match=text) as e:
            pm.draw(R, Cv, Lv, tl, tab, req, **(call or {}))
        assert "mc" in str(e.value)

    pm.draw(R, Cv, Lv, tol, icdf, abi.ac_mc_req(0, -1, 3, True, 5))
    refused("struct_bytes", struct_bytes=32)
    refused("reserved", reserved=1)
    refused("log2K", log2K=13)
    refused("log2K", log2K=-1)
    refused("bad counts", call=dict(n_inst=0))
    refused("bad counts", call=dict(nR=-1))
    refused("16384", call=dict(n_inst=16385))
    refused("null buffer", tl=None)
    refused("null buffer", tab=None)
    refused("null buffer", call=dict(have_work=False))
    refused("workspace", call=dict(work_bytes=8))
    for bad in (-1e-3, math.nan, math.inf):
        t = tol.copy()
        t[-1] = bad
        refused("tolerance", tl=t)
    t = tol.copy()
    t[0] = 1.0 / np.abs(icdf).max()
    refused(">= 1", tl=t)
    for j, bad in ((8, math.nan), (0, -math.inf), (4, icdf[3] - 1e-9)):
        tab = icdf.copy()
        tab[j] = bad
        refused("table", tab=tab)
    with pytest.raises(pm.Refused, match="no element"):
        pm.draw(np.zeros((3, 0)), np.zeros((3, 0)), np.zeros((3, 0)), np.zeros(0), icdf, abi.ac_mc_req(0, -1, 3, True, 5))
    with pytest.raises(pm.Refused, match="null request"):
        pm.draw(R, Cv, Lv, tol, icdf, None)
    W = pm.lib().spicey_mc_host_workspace_bytes
    assert W(0, 5, 7, 3, 2) == -1 and W(2, 0, 7, 3, 2) == -1 and W(2, 5, 0, 3, 2) == -1 and W(2, 5, 7, 13, 2) == -1 and W(2, 5, 7, 3, -1) == -1
    assert W(16385, 5, 7, 3, 2) == -1 and W(16384, 5, 7, 3, 2) >= 16384 * 5 * 8


# ---- the reduction ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ni", pm.REDUCE_NI)
@pytest.mark.parametrize("nf", pm.REDUCE_NF)
def test_reduction_is_the_reference_bit_for_bit(ni, nf):
    """The three forms of the output pair; no, one, every third and all but one sample invalid; a NaN, an inf and equal values among
    the valid; no mask, only lo, both; ranks at 0, n_valid - 1 and repeated; the sorting workgroup's size does not show."""
    v = pm.sweep_like(ni, nf, 3, seed=1000 * ni + nf)
    n_checked = 0
    for j, (op, on) in enumerate(pm.PAIRS):
        req = abi.ac_mc_req(op, on, 0, False, 0)
        for kind in pm.VALIDITY:
            valid = pm.validity(kind, ni)
            n_valid = ni if valid is None else int(valid.sum())
            if n_valid == 0:
                continue
            ranks = pm.rank_cases(n_valid)
            for mk in pm.MASKS:
                lo, hi = pm.limits(mk, nf, seed=j)
                sample, freq = pm.reduce(v, req, valid, lo, hi, ranks)
                rs, rf = reduce_reference_mc(v, op, on, valid, lo, hi, ranks)
                assert (sample == rs).all(), (ni, nf, op, on, kind, mk)
                assert freq.shape == rf.shape and pm.bits_equal(freq, rf).all(), (ni, nf, op, on, kind, mk)
                n_checked += 1
                # invalid samples are {-1, -1} and leave the counts; without a mask nothing violates
                bad = np.zeros(ni, bool) if valid is None else valid == 0
                assert (sample[bad] == -1).all() and (sample[~bad, 0] >= 0).all()
                assert (freq[:, 0] == n_valid).all() and freq[:, 1].sum() == sample[~bad, 0].sum()
                if mk == "none":
                    assert (sample[~bad] == [0, -1]).all()
                with np.errstate(invalid="ignore"):
                    assert (freq[:, 4] <= freq[:, 5]).all() or np.isnan(freq[:, 5]).any()
                assert pm.bits_equal(freq[:, 6], freq[:, 7]).all()
        if ni in (65, 1025):
            valid = pm.validity("third", ni)
            ranks = pm.rank_cases(int(valid.sum()))
            lo, hi = pm.limits("both", nf)
            ref = pm.reduce(v, req, valid, lo, hi, ranks)
            for threads in (64, 192, 1024):
                got = pm.reduce(v, req, valid, lo, hi, ranks, threads=threads)
                assert (got[0] == ref[0]).all() and pm.bits_equal(got[1], ref[1]).all()
    assert n_checked >= (18 if ni == 1 else 45)


def test_reduction_statistics_are_what_numpy_says():
    """Away from the lane order: the order statistics are np.sort's, the sums np.sum's to rounding."""
    ni, nf = 777, 5
    v = pm.sweep_like(ni, nf, 2, seed=3, plant=False)
    ranks = mc_ranks((0.0, 0.5, 1.0), ni)
    sample, freq = pm.reduce(v, abi.ac_mc_req(0, 1, 0, False, 0), None, None, None, ranks)
    q = np.abs(v[:, :, 0] - v[:, :, 1]) ** 2
    srt = np.sort(q, axis=0)
    assert np.allclose(freq[:, 4:], srt[ranks].T, rtol=1e-14) and np.allclose(freq[:, 2], q.sum(axis=0), rtol=1e-13)
    assert np.allclose(freq[:, 3], (q * q).sum(axis=0), rtol=1e-13)
    assert (np.diff(freq[:, 4:], axis=1) >= 0).all() and (sample == [0, -1]).all()


def test_reduction_refusals():
    v = pm.sweep_like(5, 4, 3, seed=11, plant=False)
    ranks = np.array([0, 4], np.int64)

    def refused(text, call=None, rk=ranks, valid=None, **kw):
        req = abi.ac_mc_req(kw.pop("out_p", 0), kw.pop("out_n", -1), 0, False, 0)
        for k, val in kw.items():
            setattr(req, k, val)
        with pytest.raises(pm.Refused, match=text) as e:
            pm.reduce(v, req, valid, None, None, rk, **(call or {}))
        assert "mc" in str(e.value)

    pm.reduce(v, abi.ac_mc_req(0, -1, 0, False, 0), None, None, None, ranks)
    refused("column out of range", out_p=3)
    refused("column out of range", out_n=-2)
    refused("one node twice", out_p=1, out_n=1)
    refused("one node twice", out_p=-1, out_n=-1)
    refused("struct_bytes", struct_bytes=48)
    refused("reserved", reserved=-1)
    refused("log2K", log2K=20)
    refused("bad counts", call=dict(n_inst=0))
    refused("bad counts", call=dict(n_freq=0))
    refused("bad counts", call=dict(n_v=0))
    refused("16384", call=dict(n_inst=16385))
    refused("null buffer", call=dict(have_out=False))
    refused("null buffer", call=dict(have_ranks=False))
    refused("workspace", call=dict(work_bytes=8))
    refused("rank", rk=np.array([0, 5], np.int64))
    refused("rank", rk=np.array([-1], np.int64))
    refused("rank", rk=np.array([4], np.int64), valid=np.array([1, 1, 0, 1, 1], np.uint8))
    with pytest.raises(pm.Refused, match="null request"):
        pm.reduce(v, None, None, None, None, ranks)
    # no valid sample: nothing to rank, and without ranks the counts are zeros
    none = np.zeros(5, np.uint8)
    refused("rank", rk=np.array([0], np.int64), valid=none)
    sample, freq = pm.reduce(v, abi.ac_mc_req(0, -1, 0, False, 0), none, None, None, ())
    assert (sample == -1).all() and (freq == 0).all()


# ---- against the oracle and closed forms ----------------------------------------------------------------------------------
def _variant_flat(ckt, values):
    flat = abi.flatten(ckt)
    flat.R_val[0] = [values[r.name] for r in ckt.R]
    flat.C_val[0] = [values[c.name] for c in ckt.C]
    flat.L_val[0] = [values[l.name] for l in ckt.L]
    return flat


def test_reduction_of_the_oracles_sweeps_of_the_drawn_variants(oracle_backend):
    """ac_rlc with 16 samples: the unchanged oracle sweeps every mc_values variant; numpy and the harness reduce those sweeps to
    the same bits, and mc_values is the batched draw row by row."""
    g = load_golden("ac_rlc")
    ckt = parseNetlist(golden_netlist(g))
    n, seed, tol = 16, 42, {"R": 0.02, "C": 0.05, "L": 0.1}
    freqs = np.asarray(g["freqs"], dtype=np.float64)[::3]
    vph = source_phasors(ckt)
    flats = [_variant_flat(ckt, mc_values(ckt, tol, seed, s)) for s in range(n)]
    assert pm.bits_equal(flats[0].R_val, abi.flatten(ckt).R_val).all() and not pm.bits_equal(flats[1].C_val, flats[0].C_val).all()
    # the batched draw gives the rows mc_values gives one by one
    from spicey_amd.mc import _resolve
    _, t, icdf, log2K = _resolve(ckt, tol, "gauss", 3)
    nom = abi.flatten(ckt).replicate(n)
    rinv, cv, lv = draw_reference_mc(nom.R_val, nom.C_val, nom.L_val, t, icdf, log2K, seed, True)
    stack = abi.stack_instances(flats)
    assert pm.bits_equal(rinv, 1.0 / stack.R_val).all() and pm.bits_equal(cv, stack.C_val).all() and pm.bits_equal(lv, stack.L_val).all()
    sweeps = np.stack([oracle_backend.run_ac(f, freqs, vph)["out_v"][0] for f in flats])
    n_out = sweeps.shape[2]
    ranks = mc_ranks((0.01, 0.5, 0.99), n)
    lo = np.full(len(freqs), 0.25)
    for op, on in ((n_out - 1, -1), (0, n_out - 1)):
        sample, freq = pm.reduce(sweeps, abi.ac_mc_req(op, on, log2K, True, seed), None, lo, None, ranks)
        rs, rf = reduce_reference_mc(sweeps, op, on, None, lo, None, ranks)
        assert (sample == rs).all() and pm.bits_equal(freq, rf).all()
        assert np.isfinite(freq).all() and (freq[:, 4] <= freq[:, 9]).all() and (freq[:, 4] < freq[:, 9]).any()


_rc_closed_form = pm.rc_closed_form


@pytest.mark.parametrize("resident", (False, True), ids=("per_solve", "resident"))
@pytest.mark.parametrize("dist", ("gauss", "uniform"))
def test_rc_low_pass_quantiles_against_the_closed_form(resident, dist):
    ckt = parseNetlist(RC)
    tol, n, seed, probs = {"R1": 0.01, "C": 0.05}, 97, 9, (0.0, 0.01, 0.5, 0.99, 1.0)
    r = simulateMonteCarlo(ckt, "v(out)", tol=tol, n=n, seed=seed, dist=dist, quantiles=probs, backend=pm.HostMcBackend(resident=resident))
    q, curves = _rc_closed_form(ckt, tol, seed, n, r["freq"], probs, dist)
    assert r["n"] == n and r["n_valid"] == n and r["yield"] == 1.0 and r["failing"] == [] and r["viol_per_freq"] == [0] * len(r["freq"])
    for p, ref in zip(probs, curves):
        got = np.array(r["mag"][p])
        assert (np.abs(got - ref) <= 3e-9 * np.abs(ref) + 1e-12).all(), (p, np.abs(got - ref).max())
    w = 2 * np.pi * np.array(r["freq"])
    h = 1 / (1 + 1j * w * 1e-6)
    assert (np.abs(np.array(r["nominal"]) - h) <= 3e-9 * np.abs(h) + 1e-12).all()
    assert (np.abs(np.array(r["mean2"]) - q.mean(axis=0)) <= 3e-9 * q.mean(axis=0) + 1e-12).all()
    # (the variance is a difference of two moments, each a sum of n terms rounded at 2^-53 relative: n 2^-52 mean^2 at the worst)
    assert (np.abs(np.array(r["std2"]) ** 2 - q.var(axis=0)) <= n * 2.0 ** -52 * q.mean(axis=0) ** 2 + 1e-24).all()
    # the band opens towards the corner and beyond it: 5 % on C is up to 10 % on |H|^2 there
    assert r["mag"][1.0][0] - r["mag"][0.0][0] < 1e-4 and r["mag"][1.0][-1] / r["mag"][0.0][-1] > 1.05


def test_mask_yield_and_failing_samples():
    ckt = parseNetlist(RC)
    tol, n, seed = {"R1": 0.01, "C": 0.05}, 64, 3
    fc = 1 / (2 * math.pi * 1e-6)
    # a floor that cuts through the band at the corner frequency: |H| = 0.7071 nominally
    mask = [(1.2e5, 2.0e5, 0.70, None), (1e3, 1e4, None, 1.0 + 1e-9)]
    r = simulateMonteCarlo(ckt, "v(out)", tol=tol, n=n, seed=seed, mask=mask, backend=pm.HostMcBackend())
    f = np.array(r["freq"])
    q, _ = _rc_closed_form(ckt, tol, seed, n, f, ())
    sel = (f >= 1.2e5) & (f <= 2.0e5)
    assert sel.sum() == 1 and abs(f[sel][0] - fc) < 1e4
    viol = np.zeros_like(q, bool)
    viol[:, sel] = q[:, sel] < 0.70 * 0.70
    assert 0 < viol.any(axis=1).sum() < n  # (the mask does cut through the band)
    assert r["viol_per_freq"] == viol.sum(axis=0).tolist()
    assert r["yield"] == 1.0 - viol.any(axis=1).sum() / n
    want = [(int(s), int(viol[s].sum()), float(f[int(np.argmax(viol[s]))])) for s in np.nonzero(viol.any(axis=1))[0]]
    assert r["failing"] == want and all(s != 0 for s, _, _ in want)
    # a failing sample rebuilt as a circuit violates at the frequency reported
    s, _, f_bad = want[0]
    vals = mc_values(ckt, tol, seed, s)
    assert 1.0 / (1.0 + (2 * math.pi * f_bad * vals["R1"] * vals["C1"]) ** 2) < 0.49


def test_interface_refusals():
    ckt = parseNetlist(RC)
    be = pm.HostMcBackend()
    assert simulateMonteCarlo(parseNetlist("V1 in 0 AC 1\nR1 in 0 1\n.end\n"), "v(in)", backend=be) is None
    for kw, text in ((dict(n=0), "n must be"), (dict(n=16385), "n must be"), (dict(output="i(R1)"), "output must be"), (dict(output="v(out,out)"), "twice"),
                     (dict(quantiles=(1.5,)), "quantile"), (dict(tol={"R9": 0.1}), "neither"), (dict(tol=-0.1), "tolerance"), (dict(tol=1.0), ">= 1"),
                     (dict(dist="cauchy"), "dist must be"), (dict(dist=[0.0, 1.0, 2.0, 3.0]), "2\\^L \\+ 1"), (dict(dist=[1.0, 0.0]), "non-decreasing"),
                     (dict(mask=[(1e3, 1e4, 0.5)]), "mask band"), (dict(mask=[(1e4, 1e3, 0.5, None)]), "f_from > f_to")):
        with pytest.raises(ValueError, match=text):
            simulateMonteCarlo(ckt, **{"output": "v(out)", "n": 4, "backend": be, **kw})
    with pytest.raises(TypeError, match="run_ac_mc"):
        simulateMonteCarlo(ckt, "v(out)", n=4, backend=object())
    # a user's own table: two points, everything at +tol or between
    r = simulateMonteCarlo(ckt, "v(out)", tol=0.05, n=8, dist=[0.0, 0.5, 1.0], quantiles=(0.5,), backend=be)
    assert r["n_valid"] == 8 and all(v >= 1000.0 for v in (mc_values(ckt, 0.05, 0, s, dist=[0.0, 0.5, 1.0])["R1"] for s in range(8)))
