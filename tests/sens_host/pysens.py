"""ctypes view of the CPU harness of the AC sensitivity analysis (tests/sens_host/harness.cpp): the reduction of sens_exec.h,
the two sweeps through the injected host sweep of tests/noise_host, plus the inputs the host and GPU tests share."""
import ctypes as C
import os

import numpy as np

import harness_build
from noise_host import pynoise as pn
from noise_host.pynoise import SENTINEL, Refused, bits_equal  # noqa: F401  (the tests' names for them)
from spicey_amd import abi

HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None

# (nR, nC, nL): nE = 1, 63, 64, 65, 130 with the kind borders inside a wave
REDUCTION_SHAPES = ((1, 0, 0), (20, 21, 22), (64, 0, 0), (0, 33, 32), (60, 40, 30))
REDUCTION_NF = (1, 2, 17)
# (out_p, out_n): a node against ground, a pair, ground against a node
REDUCTION_PAIRS = ((1, -1), (0, 2), (-1, 1))


def windows(nf):
    """The whole sweep, one frequency, the last two."""
    return sorted({(0, -1), (nf // 2, nf // 2), (max(nf - 2, 0), nf - 1)})


def lib():
    global _LIB
    if _LIB is None:
        L = harness_build.load(HERE, "libspicey_sens_host.so")
        vp, i32, i64 = C.c_void_p, C.c_int32, C.c_int64
        L.spicey_sens_host_workspace_bytes.restype = i64
        L.spicey_sens_host_workspace_bytes.argtypes = [i32, i64, i32]
        L.spicey_sens_host_req_bytes.restype = i32
        L.spicey_sens_host_run.restype = i32
        L.spicey_sens_host_run.argtypes = [i32, i64, vp, i32, vp, vp, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, i32, i64, C.c_char_p, i32]
        assert L.spicey_sens_host_req_bytes() == C.sizeof(abi.SpiceyAcSensReq)
        _LIB = L
    return _LIB


def _ptr(a, count):
    return a.ctypes.data if count else None


def reduce(out_v, i_dir, i_adj, R, Cv, Lv, tol, freqs, req, full=False, n_inst=None, n_freq=None, have_out=True, have_tol=True, work_bytes=-1):
    """(spec, peak, full or None) of the harness for the plain sweep's complex out_v [ni][nf][n_v] and out_i [ni][nf][n_i], the
    injected sweep's out_i, R / Cv / Lv [ni][n<kind>], tol [nE] and a request abi.ac_sens_req(...).  n_inst, n_freq, have_out,
    have_tol, work_bytes: what the call states instead of the arrays' own (the refusals).  A refusal raises Refused with the
    judge's text, after checking that the results kept their sentinel."""
    L = lib()
    out_v = np.ascontiguousarray(out_v, dtype=np.complex128)
    i_dir = np.ascontiguousarray(i_dir, dtype=np.complex128)
    i_adj = np.ascontiguousarray(i_adj, dtype=np.complex128)
    ni = i_dir.shape[0] if n_inst is None else n_inst
    nf = i_dir.shape[1] if n_freq is None else n_freq
    R, Cv, Lv = (np.ascontiguousarray(a, dtype=np.float64).reshape(i_dir.shape[0], -1) for a in (R, Cv, Lv))
    tol = np.ascontiguousarray(tol, dtype=np.float64)
    freqs = np.ascontiguousarray(freqs, dtype=np.float64)
    nE = max(len(tol), 1)
    spec = np.full((max(ni, 1), max(nf, 1), abi.SENS_SPEC), SENTINEL)
    peak = np.full((max(ni, 1), nE, abi.SENS_PEAK), SENTINEL)
    fl = np.full((max(ni, 1), max(nf, 1), nE, 2), SENTINEL) if full else None
    err = C.create_string_buffer(256)
    rc = L.spicey_sens_host_run(ni, nf, out_v.ctypes.data, out_v.shape[2], i_dir.ctypes.data, i_adj.ctypes.data, i_dir.shape[2], _ptr(R, R.size), _ptr(Cv, Cv.size),
                                _ptr(Lv, Lv.size), tol.ctypes.data if have_tol else None, freqs.ctypes.data, C.addressof(req) if req is not None else None,
                                spec.ctypes.data, peak.ctypes.data, fl.ctypes.data if full else None, int(have_out), work_bytes, err, 256)
    if rc != abi.OK:
        assert rc == abi.ERR_BAD_DESC and (spec == SENTINEL).all() and (peak == SENTINEL).all() and (fl is None or (fl == SENTINEL).all())
        raise Refused(err.value.decode())
    return spec, peak, fl


def sweep(flat, freqs, vph, node_p=0, node_n=0, amp=1.0, **kw):
    """The host sweep of tests/noise_host (pynoise.sweep): plain with vph and no nodes, injected with vph None."""
    return pn.sweep(flat, freqs, vph, node_p, node_n, amp, **kw)


def merged_status(d, x):
    """(status, inst_status, first_freq, detail) of a sens run from the results of its two host sweeps: a slot's word is D's
    where nonzero, else X's; an instance answers with the code of its lowest failing frequency index."""
    st = np.where(d["slot_status"] != 0, d["slot_status"], x["slot_status"])
    ni = st.shape[0]
    inst = np.zeros(ni, np.int32)
    first = np.full(ni, -1, np.int64)
    for j in np.nonzero((st != 0).any(axis=1))[0]:
        first[j] = int(np.argmax(st[j] != 0))
        inst[j] = abi.ERR_SINGULAR if st[j, first[j]] == 1 else abi.ERR_COMPLEX_DIV
    bad = np.nonzero(inst)[0]
    rc = int(inst[bad[0]]) if len(bad) else abi.OK
    return rc, inst, first, "" if rc == abi.OK else f"host sweep status {rc} at inst {int(bad[0])} frequency index {int(first[bad[0]])}"


class HostSensBackend:
    """run_ac_sens of a backend on the CPU: the harness's two sweeps, then its reduction.  `launches` lists the instance
    count of every call, like HipBackend.ac_launches."""

    def __init__(self, T=64, resident=False):
        self.T, self.resident = T, resident
        self.launches = []

    def run_ac_sens(self, flat, freqs, vph, node_p, node_n, req, tol, full=False):
        self.launches.append(flat.n_inst)
        d = sweep(flat, freqs, vph, T=self.T, resident=self.resident)
        x = sweep(flat, freqs, None, node_p, node_n, 1.0, T=self.T, resident=self.resident)
        for r in (d, x):  # (what no sweep answers: a structurally singular circuit, a refused call)
            if r["status"] not in (abi.OK, abi.ERR_SINGULAR, abi.ERR_COMPLEX_DIV) or (r["status"] != abi.OK and not r["slot_status"].any()):
                return r
        rc, inst, first, detail = merged_status(d, x)
        res = {"status": rc, "detail": detail, "inst_status": inst, "first_freq": first, "dir": d, "adj": x}
        with np.errstate(all="ignore"):
            res["spec"], res["peak"], res["full"] = reduce(d["out_v"], d["out_i"], x["out_i"], flat.R_val, flat.C_val, flat.L_val, tol, freqs, req, full=full)
        return res


def sens_inputs(n_inst, n_freq, shape, n_extra, n_v, seed):
    """Seeded inputs of the reduction: currents and voltages of both signs over several decades, element values that differ per
    instance, tolerances with zeros among them, ascending frequencies of uneven spacing."""
    rng = np.random.default_rng(seed)
    nR, nC, nL = shape
    nE = nR + nC + nL
    n_i = nE + n_extra

    def cx(shape):
        mag = 10.0 ** rng.uniform(-6, 1, shape)
        return mag * np.exp(1j * rng.uniform(0, 2 * np.pi, shape))
    i_dir, i_adj, out_v = cx((n_inst, n_freq, n_i)), cx((n_inst, n_freq, n_i)), cx((n_inst, n_freq, n_v))
    scale = (1.0 + 0.37 * np.arange(n_inst))[:, None]
    R = 10.0 ** rng.uniform(0, 6, (n_inst, nR)) * scale
    Cv = 10.0 ** rng.uniform(-12, -6, (n_inst, nC)) * scale
    Lv = 10.0 ** rng.uniform(-9, -3, (n_inst, nL)) * scale
    tol = 10.0 ** rng.uniform(-3, -1, nE)
    tol[rng.random(nE) < 0.2] = 0.0
    tol[nE // 2] = 0.0
    freqs = np.cumsum(10.0 ** rng.uniform(0, 5, n_freq))
    return out_v, i_dir, i_adj, R, Cv, Lv, tol, freqs
