"""simulateMonteCarlo(): the distribution of an AC response under component tolerances — SPICE's .mc.

n samples of the circuit, each with its R, C and L drawn around the nominal values, are the instances of ONE batched sweep of the
AC engine.  The values are drawn on the device (spicey_ac_run_mc, include/spicey_hip.h), the sweep reads them there and its
results stay there, and a reduction ACROSS the instances — an LDS sort per frequency — brings back a few doubles per frequency:
order statistics for the requested quantiles, the sum and the sum of squares of |H|^2, the count of samples outside a spec mask,
and per sample the number of frequencies at which it violates the mask.  Unlike the first-order bounds of simulateSens this is
the response's actual distribution: a Q = 30 notch is not linear in a 5 % capacitor.

    simulateMonteCarlo(ckt, output="v(out)", tol={"R": 0.01, "C": 0.05}, n=1024, seed=0, dist="gauss", nsigma=3,
                       quantiles=(0.01, 0.5, 0.99), mask=None, freqs=None, exact_order=False)

tol resolves like simulateSens's (a float for every element, or a dict of element names and the kind keys "R", "C", "L"; None:
the default {"R": 0.01, "C": 0.05}).  dist: "uniform" (value = nom (1 + tol u), u uniform in [-1, 1]), "gauss" (tol is
nsigma standard deviations, truncated there) or an array: a table icdf[2^L + 1] of the inverse distribution function in units of
the tolerance, finite and non-decreasing.  mask: bands (f_from, f_to, min_mag, max_mag) of |H| (None: no limit on that side),
squared and laid on the frequency grid here.  Sample 0 is always the nominal circuit.

The draw is integer arithmetic — Philox4x32-10 under counter (sample, element, 0, 0) and key seed, 52 bits interpolating a host-built
table — so draw_reference_mc() below, plain numpy, gives the device's bits, and mc_values(ckt, tol, seed, s) the element values
of sample s: a failing sample can be rebuilt and inspected as a circuit.  reduce_reference_mc() is the reduction in numpy
(view(np.uint64), np.sort).

The result dict:
    freq, nominal          the frequencies and the complex H of the nominal circuit (sample 0)
    mag                    {p: [n_freq]}: |H| at probability p — the order statistics of |H|^2 at floor(p (n_valid - 1)) and the
                           next rank, interpolated, then square-rooted
    mean2, std2            mean and standard deviation of |H|^2 per frequency
    n, n_valid             samples drawn, samples whose every solve succeeded (the others leave every statistic)
    yield                  the fraction of valid samples that meet the mask at every frequency (1.0 without a mask)
    viol_per_freq          valid samples outside the mask, per frequency
    failing                [(sample, violating frequencies, first violating frequency)], ascending sample index
"""
from __future__ import annotations

import math
from statistics import NormalDist
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import abi
from .ac import _check_resistors, source_phasors
from .ac_batch import batch_backend, slot_error
from .measure import _parse_signal
from .netlist import ParsedCircuit
from .noise import _freqs_of
from .sens import _elements, _tolerances

LANES = 64
_M0, _M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
_W0, _W1 = 0x9E3779B9, 0xBB67AE85
_LO32 = np.uint64(0xFFFFFFFF)
_SH32 = np.uint64(32)
_ABS = np.uint64(0x7FFFFFFFFFFFFFFF)


def philox4x32(counter, key) -> np.ndarray:
    """Philox4x32-10 of counters [..., 4] under key (k0, k1) -> uint32 [..., 4]."""
    c = np.asarray(counter, dtype=np.uint64) & _LO32
    c0, c1, c2, c3 = (c[..., j].copy() for j in range(4))
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = _M0 * c0, _M1 * c2
        c0, c1, c2, c3 = (p1 >> _SH32) ^ c1 ^ np.uint64(k0), p1 & _LO32, (p0 >> _SH32) ^ c3 ^ np.uint64(k1), p0 & _LO32
        k0, k1 = (k0 + _W0) & 0xFFFFFFFF, (k1 + _W1) & 0xFFFFFFFF
    return np.stack([c0, c1, c2, c3], axis=-1).astype(np.uint32)


def mc_uniform(seed: int, n_inst: int, nE: int) -> np.ndarray:
    """m [n_inst][nE] uint64: the 52 uniform bits of every (sample, element)."""
    c = np.zeros((n_inst, nE, 4), np.uint64)
    c[:, :, 0] = np.arange(n_inst, dtype=np.uint64)[:, None]
    c[:, :, 1] = np.arange(nE, dtype=np.uint64)[None, :]
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    x = philox4x32(c, (seed & 0xFFFFFFFF, seed >> 32)).astype(np.uint64)
    return (x[:, :, 0] << np.uint64(20)) | (x[:, :, 1] >> np.uint64(12))


def icdf_table(dist="gauss", nsigma: float = 3) -> Tuple[np.ndarray, int]:
    """(icdf [2^L + 1], L): the inverse distribution function in units of the tolerance, built with the host's libm."""
    if isinstance(dist, str):
        if dist == "uniform":
            return np.array([-1.0, 1.0]), 0
        if dist != "gauss":
            raise ValueError(f"simulateMonteCarlo: dist must be 'uniform', 'gauss' or a table, got {dist!r}")
        if not (isinstance(nsigma, (int, float)) and math.isfinite(nsigma) and nsigma > 0):
            raise ValueError(f"simulateMonteCarlo: nsigma must be a finite number > 0, got {nsigma!r}")
        K, nd, ns = 1024, NormalDist(), float(nsigma)
        tab = np.empty(K + 1)
        tab[0], tab[K] = -1.0, 1.0
        for j in range(1, K):
            tab[j] = min(max(nd.inv_cdf(j / K), -ns), ns) / ns
        return tab, 10
    tab = np.ascontiguousarray(dist, dtype=np.float64).reshape(-1)
    L = int(tab.size - 1).bit_length() - 1 if tab.size >= 2 else -1
    if L < 0 or L > abi.MC_MAX_LOG2K or tab.size != (1 << L) + 1:
        raise ValueError(f"simulateMonteCarlo: a table has 2^L + 1 entries, L in [0, {abi.MC_MAX_LOG2K}], got {tab.size}")
    if not np.isfinite(tab).all() or (np.diff(tab) < 0).any():
        raise ValueError("simulateMonteCarlo: a table must be finite and non-decreasing")
    return tab, L


def mc_deviates(m: np.ndarray, icdf: np.ndarray, log2K: int) -> np.ndarray:
    """d of the 52-bit integers m: the table interpolated — one subtraction, one product, one addition, each rounded."""
    sh = 52 - int(log2K)
    j = (m >> np.uint64(sh)).astype(np.int64)
    r = m & np.uint64((1 << sh) - 1)
    frac = r.astype(np.float64) * np.float64(2.0 ** -sh)
    a = icdf[j]
    step = icdf[j + 1] - a
    return a + frac * step


def mc_gains(n_inst: int, tol, icdf, log2K: int, seed: int, keep_first: bool = True) -> np.ndarray:
    """g [n_inst][nE] = 1 + tol d: the factor every element of every sample takes (sample 0: 1.0 with keep_first)."""
    tol = np.asarray(tol, dtype=np.float64).reshape(-1)
    d = mc_deviates(mc_uniform(seed, n_inst, len(tol)), np.asarray(icdf, dtype=np.float64).reshape(-1), log2K)
    g = 1.0 + tol[None, :] * d
    if keep_first:
        g[0, :] = 1.0
    return g


def draw_reference_mc(R, Cv, Lv, tol, icdf, log2K: int, seed: int, keep_first: bool = True):
    """The definition of spicey_ac_mc_draw_device in numpy: nominal R (ohms), Cv, Lv [n_inst][n<kind>], tol [nE] ->
    (1 / R', C', L') of the same shapes, the arrays a sweep reads."""
    ni = np.asarray(R).shape[0]
    R, Cv, Lv = (np.asarray(a, dtype=np.float64).reshape(ni, -1) for a in (R, Cv, Lv))
    tol = np.asarray(tol, dtype=np.float64).reshape(-1)
    icdf = np.asarray(icdf, dtype=np.float64).reshape(-1)
    nR, nC, nL = R.shape[1], Cv.shape[1], Lv.shape[1]
    nE = nR + nC + nL
    if len(tol) != nE or icdf.size != (1 << log2K) + 1:
        raise ValueError("draw_reference_mc: tol has one entry per element, icdf 2^log2K + 1")
    g = mc_gains(ni, tol, icdf, log2K, seed, keep_first)
    return 1.0 / (R * g[:, :nR]), Cv * g[:, nR:nR + nC], Lv * g[:, nR + nC:]


def _lane_sum(x: np.ndarray) -> np.ndarray:
    """x [n_freq][n] -> [n_freq]: lane l adds x[l], x[l + 64], ... in ascending index to +0.0, the 64 partials meet by
    s[l] += s[l + stride] for stride = 32 .. 1."""
    nf, n = x.shape
    groups = (n + LANES - 1) // LANES
    pad = np.zeros((nf, max(groups, 1) * LANES))
    pad[:, :n] = x
    pad = pad.reshape(nf, max(groups, 1), LANES)
    s = np.zeros((nf, LANES))
    for g in range(groups):
        s = s + pad[:, g, :]  # (a lane past the last value adds +0.0: no change to a sum that is >= 0 or NaN)
    stride = LANES // 2
    while stride:
        s[:, :stride] = s[:, :stride] + s[:, stride:2 * stride]
        stride //= 2
    return s[:, 0]


def reduce_reference_mc(out_v, out_p: int, out_n: int, valid=None, lo=None, hi=None, ranks=()):
    """The definition of spicey_ac_mc_reduce_device in numpy: out_v complex [n_inst][n_freq][n_v] -> (sample [n_inst][2] int64,
    freq [n_freq][4 + n_rank])."""
    v = np.asarray(out_v, dtype=np.complex128)
    ni, nf = v.shape[0], v.shape[1]
    ok = np.ones(ni, bool) if valid is None else np.asarray(valid).astype(bool).reshape(ni)
    ranks = np.asarray(ranks, dtype=np.int64).reshape(-1)
    n_valid = int(ok.sum())
    if out_p == out_n or (len(ranks) and (ranks.min() < 0 or ranks.max() >= n_valid)):
        raise ValueError("reduce_reference_mc: bad request")
    with np.errstate(all="ignore"):
        re, im = np.zeros((ni, nf)), np.zeros((ni, nf))
        if out_p >= 0:
            re, im = v[:, :, out_p].real.copy(), v[:, :, out_p].imag.copy()
        if out_n >= 0:
            re, im = re - v[:, :, out_n].real, im - v[:, :, out_n].imag
        q = re * re + im * im
        if lo is None and hi is None:
            viol = np.zeros((ni, nf), bool)
        else:
            lo_ = np.full(nf, -np.inf) if lo is None else np.asarray(lo, dtype=np.float64)
            hi_ = np.full(nf, np.inf) if hi is None else np.asarray(hi, dtype=np.float64)
            viol = ~((q >= lo_[None, :]) & (q <= hi_[None, :]))
        sample = np.full((ni, 2), -1, np.int64)
        cnt = viol.sum(axis=1)
        first = np.where(cnt > 0, viol.argmax(axis=1), -1)
        sample[ok, 0], sample[ok, 1] = cnt[ok], first[ok]
        keys = np.ascontiguousarray(q[ok].T).view(np.uint64) & _ABS  # [n_freq][n_valid]
        x = np.sort(keys, axis=1).view(np.float64)
        freq = np.zeros((nf, abi.MC_FREQ_HEAD + len(ranks)))
        freq[:, 0] = float(n_valid)
        freq[:, 1] = viol[ok].sum(axis=0)
        freq[:, 2] = _lane_sum(x)
        freq[:, 3] = _lane_sum(x * x)
        if len(ranks):
            freq[:, abi.MC_FREQ_HEAD:] = x[:, ranks]
    return sample, freq


def mc_ranks(probs, n_valid: int) -> np.ndarray:
    """The ranks spicey_ac_run_mc reduces for `probs`: floor(p (n_valid - 1)) and the next, capped at n_valid - 1."""
    out = []
    for p in probs:
        r = int(math.floor(float(p) * float(n_valid - 1)))
        out += [r, min(r + 1, n_valid - 1)]
    return np.asarray(out, dtype=np.int64)


def _resolve(ckt: ParsedCircuit, tol, dist, nsigma):
    elements = _elements(ckt)
    if not elements:
        raise ValueError("simulateMonteCarlo: the circuit has no R, C or L, so there is nothing to vary")
    try:
        t = _tolerances(elements, 0.0 if tol is None else tol)
    except ValueError as e:
        raise ValueError(str(e).replace("simulateSens", "simulateMonteCarlo")) from None
    icdf, log2K = icdf_table(dist, nsigma)
    top = max(abs(icdf[0]), abs(icdf[-1]))
    if (t * top >= 1.0).any():
        raise ValueError("simulateMonteCarlo: tol * max|icdf| >= 1: a drawn value could be zero or negative")
    return elements, t, icdf, log2K


def mc_values(ckt: ParsedCircuit, tol, seed: int, s: int, dist="gauss", nsigma: float = 3) -> Dict[str, float]:
    """{element name: value} of sample s of simulateMonteCarlo(ckt, tol=tol, seed=seed, dist=dist, nsigma=nsigma): ohms, farads,
    henries, from the numpy draw (the resistance is R g itself, whose quotient 1.0 / (R g) the sweep reads).  Sample 0 is nominal."""
    elements, t, icdf, log2K = _resolve(ckt, tol, dist, nsigma)
    if s < 0:
        raise ValueError("mc_values: s >= 0")
    nE = len(elements)
    m = mc_uniform(seed, s + 1, nE)[s]
    g = 1.0 + t * mc_deviates(m, icdf, log2K)
    if s == 0:
        g[:] = 1.0
    return {name: float(np.float64(value) * g[e]) for e, (name, _, value) in enumerate(elements)}


def _mask_limits(mask, freqs: np.ndarray):
    """Bands (f_from, f_to, min_mag, max_mag) -> (lo, hi) [n_freq] limits of |H|^2, or (None, None) without a mask."""
    if not mask:
        return None, None
    lo, hi = np.full(len(freqs), -np.inf), np.full(len(freqs), np.inf)
    for band in mask:
        if len(band) != 4:
            raise ValueError(f"simulateMonteCarlo: a mask band is (f_from, f_to, min_mag, max_mag), got {band!r}")
        f0, f1, a, b = band
        if not (f0 <= f1):
            raise ValueError(f"simulateMonteCarlo: mask band {band!r}: f_from > f_to")
        sel = (freqs >= f0) & (freqs <= f1)
        for v in (a, b):
            if v is not None and not (isinstance(v, (int, float)) and v >= 0 and not math.isnan(v)):
                raise ValueError(f"simulateMonteCarlo: mask band {band!r}: a magnitude limit is a number >= 0 or None")
        if a is not None:
            lo[sel] = np.maximum(lo[sel], float(a) * float(a))
        if b is not None:
            hi[sel] = np.minimum(hi[sel], float(b) * float(b))
    return lo, hi


def quantile_curves(freq_stats: np.ndarray, probs: Sequence[float], n_valid: int) -> List[np.ndarray]:
    """|H| at each probability from a run's freq_stats: the two order statistics of |H|^2 interpolated, then square-rooted."""
    out = []
    for j, p in enumerate(probs):
        pos = float(p) * float(n_valid - 1)
        frac = pos - math.floor(pos)
        a, b = freq_stats[:, abi.MC_FREQ_HEAD + 2 * j], freq_stats[:, abi.MC_FREQ_HEAD + 2 * j + 1]
        with np.errstate(all="ignore"):
            out.append(np.sqrt(a + frac * (b - a)))
    return out


def simulateMonteCarlo(ckt: ParsedCircuit, output: str = "v(out)", tol=None, n: int = 1024, seed: int = 0, dist="gauss", nsigma: float = 3,
                       quantiles: Sequence[float] = (0.01, 0.5, 0.99), mask=None, freqs=None, exact_order: bool = False, *, device: int = 0,
                       backend=None) -> Optional[dict]:
    """Monte Carlo tolerance analysis of `ckt` at `output` (module text).  None without a .ac card and without freqs.  Raises what
    simulateAC raises when the nominal circuit's sweep fails; a drawn sample whose sweep fails only leaves the statistics.
    backend: a test backend with run_ac_mc(flat, freqs, vph, req, tol, icdf, lo, hi, probs)."""
    if tol is None:
        tol = {"R": 0.01, "C": 0.05}
    fr = _freqs_of(ckt, freqs)
    if fr is None:
        return None
    if not len(fr):
        raise ValueError("simulateMonteCarlo: the sweep has no frequencies")
    if isinstance(n, bool) or not isinstance(n, int) or n < 1 or n > abi.MC_MAX_INST:
        raise ValueError(f"simulateMonteCarlo: n must be an integer in [1, {abi.MC_MAX_INST}] (one workgroup sorts a frequency's samples), got {n!r}")
    if not str(output).strip().lower().startswith("v("):
        raise ValueError(f"simulateMonteCarlo: output must be v(node) or v(node,node), got {output!r}")
    _, a, b = _parse_signal(ckt, str(output), [])
    if a == b:
        raise ValueError(f"simulateMonteCarlo: {output!r}: the output pair names one node twice")
    probs = [float(p) for p in quantiles]
    if any(not (0.0 <= p <= 1.0) for p in probs):
        raise ValueError("simulateMonteCarlo: a quantile lies in [0, 1]")
    elements, t, icdf, log2K = _resolve(ckt, tol, dist, nsigma)
    lo, hi = _mask_limits(mask, fr)
    _check_resistors(ckt, fr.tolist())
    be = batch_backend(backend, exact_order, device, "simulateMonteCarlo")
    if not hasattr(be, "run_ac_mc"):
        raise TypeError("simulateMonteCarlo: the backend has no run_ac_mc")
    out_nodes = sorted({x for x in (a, b) if x != 0})
    col = {x: k for k, x in enumerate(out_nodes)}
    flat = abi.flatten(ckt)
    flat.out_nodes = np.ascontiguousarray(out_nodes, dtype=np.int32)
    req = abi.ac_mc_req(col[a] if a else -1, col[b] if b else -1, log2K, True, seed)
    res = be.run_ac_mc(flat.replicate(n), fr, source_phasors(ckt), req, t, icdf, lo, hi, probs)
    rc = res["status"]
    if rc not in (abi.OK, abi.ERR_SINGULAR, abi.ERR_COMPLEX_DIV):
        raise RuntimeError(res.get("detail") or f"spicey native error {rc}")
    ist = np.asarray(res["inst_status"])
    if int(ist[0]) != 0:  # (the nominal circuit itself fails: simulateAC's error)
        raise slot_error(int(ist[0]), res.get("detail", ""))
    stats, sample = res["freq_stats"], res["sample"]
    n_valid = int(np.count_nonzero(ist == 0))
    bad = sample[:, 0] > 0
    with np.errstate(all="ignore"):
        mean2 = stats[:, 2] / n_valid
        std2 = np.sqrt(np.maximum(stats[:, 3] / n_valid - mean2 * mean2, 0.0))
    curves = quantile_curves(stats, probs, n_valid)
    return {"freq": fr.tolist(), "nominal": res["nominal"].tolist(), "mag": {p: c.tolist() for p, c in zip(probs, curves)},
            "mean2": mean2.tolist(), "std2": std2.tolist(), "n": n, "n_valid": n_valid,
            "yield": float(np.count_nonzero((sample[:, 0] == 0))) / n_valid, "viol_per_freq": stats[:, 1].astype(np.int64).tolist(),
            "failing": [(int(s), int(sample[s, 0]), float(fr[int(sample[s, 1])])) for s in np.nonzero(bad)[0]],
            "elements": [name for name, _, _ in elements], "tol": t.tolist(), "seed": int(seed), "mc_ms": res.get("mc_ms"), "draw_ms": res.get("draw_ms"),
            "kernel_ms": res.get("kernel_ms")}
