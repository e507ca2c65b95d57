"""ctypes view of the CPU harness of the Monte Carlo tolerance analysis (tests/mc_host/harness.cpp): the draw and the reduction of
mc_exec.h, plus the inputs the host and GPU tests share."""
import ctypes as C
import os

import numpy as np

import harness_build
from noise_host.pynoise import Refused, bits_equal  # noqa: F401  (the tests' names for them)
from spicey_amd import abi

HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None

SENTINEL = -7.25
SENTINEL_I = -99
DRAW_NI = (1, 2, 65)
DRAW_L = (0, 1, 10)
REDUCE_NI = (1, 2, 63, 64, 65, 1000, 1025)
REDUCE_NF = (1, 2, 17, 65, 130)
# (out_p, out_n): a node against ground, a pair, ground against a node
PAIRS = ((1, -1), (0, 2), (-1, 1))
VALIDITY = ("none", "first", "last", "third", "all_but_one")
MASKS = ("none", "lo", "both")


def lib():
    global _LIB
    if _LIB is None:
        L = harness_build.load(HERE, "libspicey_mc_host.so")
        vp, i32, i64, u32, u64 = C.c_void_p, C.c_int32, C.c_int64, C.c_uint32, C.c_uint64
        L.spicey_mc_host_workspace_bytes.restype = i64
        L.spicey_mc_host_workspace_bytes.argtypes = [i32, i64, i32, i32, i32]
        L.spicey_mc_host_req_bytes.restype = i32
        L.spicey_mc_host_philox.restype = None
        L.spicey_mc_host_philox.argtypes = [vp, u32, u32]
        L.spicey_mc_host_uniform.restype = None
        L.spicey_mc_host_uniform.argtypes = [u64, i32, i32, vp]
        L.spicey_mc_host_draw.restype = i32
        L.spicey_mc_host_draw.argtypes = [i32, i32, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, i32, i64, C.c_char_p, i32]
        L.spicey_mc_host_sort.restype = None
        L.spicey_mc_host_sort.argtypes = [vp, i32, i32]
        L.spicey_mc_host_reduce.restype = i32
        L.spicey_mc_host_reduce.argtypes = [i32, i64, vp, i32, vp, vp, vp, vp, i32, vp, vp, vp, i32, i64, i32, C.c_char_p, i32]
        assert L.spicey_mc_host_req_bytes() == C.sizeof(abi.SpiceyAcMcReq)
        _LIB = L
    return _LIB


def _ptr(a):
    return a.ctypes.data if a is not None and a.size else None


def philox(counter, key):
    c = np.ascontiguousarray(counter, dtype=np.uint32).copy()
    lib().spicey_mc_host_philox(c.ctypes.data, int(key[0]), int(key[1]))
    return c


def uniform(seed, n_inst, nE):
    m = np.zeros((n_inst, nE), np.uint64)
    lib().spicey_mc_host_uniform(int(seed) & 0xFFFFFFFFFFFFFFFF, n_inst, nE, m.ctypes.data)
    return m


def draw(R, Cv, Lv, tol, icdf, req, n_inst=None, nR=None, have_work=True, work_bytes=-1):
    """(1 / R', C', L') of the harness for nominal R / Cv / Lv [ni][n<kind>], tol [nE], icdf and a request abi.ac_mc_req(...).
    n_inst, nR, have_work, work_bytes: what the call states instead of the arrays' own (the refusals).  tol / icdf None stand for
    null pointers.  A refusal raises Refused with the judge's text, after checking that the results kept their sentinel."""
    ni0 = np.asarray(R).shape[0]
    R, Cv, Lv = (np.ascontiguousarray(a, dtype=np.float64).reshape(ni0, -1) for a in (R, Cv, Lv))
    tol = None if tol is None else np.ascontiguousarray(tol, dtype=np.float64)
    icdf = None if icdf is None else np.ascontiguousarray(icdf, dtype=np.float64)
    oR, oC, oL = (np.full(a.shape, SENTINEL) for a in (R, Cv, Lv))
    err = C.create_string_buffer(256)
    rc = lib().spicey_mc_host_draw(ni0 if n_inst is None else n_inst, R.shape[1] if nR is None else nR, Cv.shape[1], Lv.shape[1], _ptr(R), _ptr(Cv), _ptr(Lv),
                                   None if tol is None else tol.ctypes.data, None if icdf is None else icdf.ctypes.data,
                                   C.addressof(req) if req is not None else None, _ptr(oR), _ptr(oC), _ptr(oL), int(have_work), work_bytes, err, 256)
    if rc != abi.OK:
        assert rc == abi.ERR_BAD_DESC and (oR == SENTINEL).all() and (oC == SENTINEL).all() and (oL == SENTINEL).all()
        raise Refused(err.value.decode())
    return oR, oC, oL


def reduce(out_v, req, valid=None, lo=None, hi=None, ranks=(), n_inst=None, n_freq=None, n_v=None, have_out=True, work_bytes=-1, threads=0, have_ranks=True):
    """(sample [ni][2] int64, freq [nf][4 + n_rank]) of the harness for complex out_v [ni][nf][n_v].  threads: of the sorting
    workgroup (0: the launcher's choice).  A refusal raises Refused, after checking that the results kept their sentinel."""
    out_v = np.ascontiguousarray(out_v, dtype=np.complex128)
    ni = out_v.shape[0] if n_inst is None else n_inst
    nf = out_v.shape[1] if n_freq is None else n_freq
    valid = None if valid is None else np.ascontiguousarray(valid, dtype=np.uint8)
    lo = None if lo is None else np.ascontiguousarray(lo, dtype=np.float64)
    hi = None if hi is None else np.ascontiguousarray(hi, dtype=np.float64)
    ranks = np.ascontiguousarray(ranks, dtype=np.int64).reshape(-1)
    sample = np.full((out_v.shape[0], 2), SENTINEL_I, np.int64)
    freq = np.full((out_v.shape[1], abi.MC_FREQ_HEAD + len(ranks)), SENTINEL)
    err = C.create_string_buffer(256)
    with np.errstate(all="ignore"):
        rc = lib().spicey_mc_host_reduce(ni, nf, out_v.ctypes.data, out_v.shape[2] if n_v is None else n_v, None if valid is None else valid.ctypes.data,
                                         None if lo is None else lo.ctypes.data, None if hi is None else hi.ctypes.data, _ptr(ranks) if have_ranks else None,
                                         len(ranks), C.addressof(req) if req is not None else None, sample.ctypes.data, freq.ctypes.data, int(have_out),
                                         work_bytes, threads, err, 256)
    if rc != abi.OK:
        assert rc == abi.ERR_BAD_DESC and (sample == SENTINEL_I).all() and (freq == SENTINEL).all()
        raise Refused(err.value.decode())
    return sample, freq


def validity(kind, ni):
    """The validity masks of the tests: None (all valid) or bytes [ni]."""
    v = np.ones(ni, np.uint8)
    if kind == "none":
        return None
    if kind == "first":
        v[0] = 0
    elif kind == "last":
        v[-1] = 0
    elif kind == "third":
        v[::3] = 0
    else:
        v[:] = 0
        v[ni // 2] = 1
    return v


def limits(kind, nf, seed=0):
    """(lo, hi) [nf] of |H|^2 with infinities among them, or None."""
    rng = np.random.default_rng(1000 + seed)
    lo = 10.0 ** rng.uniform(-3, -1, nf)
    hi = 10.0 ** rng.uniform(-1, 1, nf)
    lo[rng.random(nf) < 0.2] = -np.inf
    hi[rng.random(nf) < 0.2] = np.inf
    return (None, None) if kind == "none" else (lo, None) if kind == "lo" else (lo, hi)


def rank_cases(n_valid):
    """Ranks at 0, n_valid - 1, the middle, and one repeated."""
    return np.array([0, n_valid - 1, n_valid // 2, n_valid // 2, min(1, n_valid - 1)], np.int64) if n_valid > 0 else np.zeros(0, np.int64)


def drawn_flat(flat, tol, icdf, req):
    """A FlatCircuit whose rows are the numpy draw's values (ohms, farads, henries): a plain sweep of it reads 1.0 / (R g), C g
    and L g — what a Monte Carlo run's sweep reads."""
    from spicey_amd.mc import mc_gains
    out = replicate_rows(flat)
    g = mc_gains(out.n_inst, tol, icdf, req.log2K, req.seed, bool(req.keep_first))
    nR, nC = out.nR, out.nC
    out.R_val = np.ascontiguousarray(out.R_val * g[:, :nR])
    out.C_val = np.ascontiguousarray(out.C_val * g[:, nR:nR + nC])
    out.L_val = np.ascontiguousarray(out.L_val * g[:, nR + nC:])
    return out


def replicate_rows(flat):
    """A copy of `flat` with value arrays of its own."""
    arrays = {k: getattr(flat, k) for k in abi.FlatCircuit.TOPO}
    for k in abi.FlatCircuit.VALS:
        arrays[k] = getattr(flat, k).copy()
    arrays["S_ison"] = flat.S_ison.copy()
    arrays["out_nodes"] = flat.out_nodes
    return abi.FlatCircuit(flat.n_nodes, flat.n_inst, **arrays)


def run_mc_reference(run, flat, freqs, vph, req, tol, icdf, lo=None, hi=None, probs=()):
    """What AcHandle.run_mc returns, from `run(flat, freqs, vph)` (a plain sweep: a second handle's, the host sweep's, the
    oracle's) of the drawn circuit and the harness's reduction of it."""
    from spicey_amd.mc import mc_ranks
    res = run(drawn_flat(flat, tol, icdf, req), freqs, vph)
    ist = np.asarray(res["inst_status"])
    valid = (ist == 0).astype(np.uint8)
    n_valid = int(valid.sum())
    out = {"status": res["status"], "detail": res.get("detail", ""), "inst_status": ist, "first_freq": res.get("first_freq"), "sweep": res}
    if n_valid:
        out["sample"], out["freq_stats"] = reduce(res["out_v"], req, None if n_valid == len(valid) else valid, lo, hi, mc_ranks(probs, n_valid))
        h = np.zeros(len(freqs), np.complex128)
        if req.out_p >= 0:
            h = res["out_v"][0, :, req.out_p].copy()
        if req.out_n >= 0:
            h = h - res["out_v"][0, :, req.out_n]
        out["nominal"] = h if req.keep_first else None
    return out


class HostMcBackend:
    """run_ac_mc of a backend on the CPU: the numpy draw, the host sweep of tests/noise_host, the harness's reduction."""

    def __init__(self, T=64, resident=False):
        self.T, self.resident = T, resident

    def run_ac_mc(self, flat, freqs, vph, req, tol, icdf, lo=None, hi=None, probs=()):
        from noise_host import pynoise as pn
        return run_mc_reference(lambda f, fr, ph: pn.sweep(f, fr, ph, T=self.T, resident=self.resident), flat, freqs, vph, req, tol, icdf, lo, hi, probs)


def sweep_like(ni, nf, n_v, seed, plant=True):
    """Seeded complex voltages [ni][nf][n_v] over several decades; with plant a NaN and an inf in the samples the validity masks
    keep (ni // 2) and, where there are others, sample 1."""
    rng = np.random.default_rng(seed)
    mag = 10.0 ** rng.uniform(-2, 0.5, (ni, nf, n_v))
    v = mag * np.exp(1j * rng.uniform(0, 2 * np.pi, (ni, nf, n_v)))
    if plant:
        v[ni // 2, 0, :] = np.nan
        v[ni // 2, nf - 1, :] = np.inf + 0j
        if ni > 4:
            v[1, nf // 2, 1] = complex(np.inf, 1.0)
        v[0, 0, :] = v[ni - 1, 0, :]  # (equal keys)
    return v


def draw_inputs(ni, shape, log2K, seed):
    """Nominal values that differ per instance, tolerances with zeros among them, a skewed non-decreasing table with a flat run."""
    rng = np.random.default_rng(seed)
    nR, nC, nL = shape
    nE = nR + nC + nL
    scale = (1.0 + 0.37 * np.arange(ni))[:, None]
    R = 10.0 ** rng.uniform(0, 6, (ni, nR)) * scale
    Cv = 10.0 ** rng.uniform(-12, -6, (ni, nC)) * scale
    Lv = 10.0 ** rng.uniform(-9, -3, (ni, nL)) * scale
    tol = 10.0 ** rng.uniform(-3, -1, nE)
    tol[rng.random(nE) < 0.2] = 0.0
    tol[nE // 2] = 0.0
    K = 1 << log2K
    icdf = np.sort(rng.uniform(-2.0, 1.5, K + 1))
    if K >= 4:
        icdf[2] = icdf[1]
    return R, Cv, Lv, tol, icdf


def rc_closed_form(ckt, tol, seed, n, freqs, probs, dist="gauss"):
    """|H| quantiles of H = 1 / (1 + jwRC) over mc_values' samples, by the ranks and the interpolation of the run."""
    from spicey_amd import mc as _mc
    w = 2 * np.pi * np.asarray(freqs)
    q = np.zeros((n, len(w)))
    for s in range(n):
        vals = _mc.mc_values(ckt, tol, seed, s, dist=dist)
        q[s] = 1.0 / (1.0 + (w * vals["R1"] * vals["C1"]) ** 2)
    srt = np.sort(q, axis=0)
    stats = np.zeros((len(w), 4 + 2 * len(probs)))
    stats[:, 4:] = srt[_mc.mc_ranks(probs, n)].T
    return q, _mc.quantile_curves(stats, probs, n)
