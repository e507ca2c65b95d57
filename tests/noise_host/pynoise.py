"""ctypes view of the CPU harness of the noise analysis (tests/noise_host/harness.cpp): the reduction of noise_exec.h and the
injected AC sweep through the host form of ac_exec.h, plus the inputs the host and GPU tests share."""
import ctypes as C
import os

import numpy as np

import harness_build
from spicey_amd import abi

HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None
U = 2.0 ** -52
SENTINEL = -7.25

REDUCTION_NR = (1, 63, 64, 65, 130)
REDUCTION_NF = (1, 2, 17)


def lib():
    global _LIB
    if _LIB is None:
        L = harness_build.load(HERE, "libspicey_noise_host.so")
        vp, i32, i64, f64 = C.c_void_p, C.c_int32, C.c_int64, C.c_double
        L.spicey_noise_host_workspace_bytes.restype = i64
        L.spicey_noise_host_workspace_bytes.argtypes = [i32, i64, i32]
        L.spicey_noise_host_req_bytes.restype = i32
        L.spicey_noise_host_run.restype = i32
        L.spicey_noise_host_run.argtypes = [i32, i64, vp, i32, vp, i32, vp, i32, vp, vp, vp, vp, vp, i32, i64, C.c_char_p, i32]
        L.spicey_noise_host_sweep.restype = i32
        L.spicey_noise_host_sweep.argtypes = [C.POINTER(abi.SpiceyDesc), i32, i64, vp, vp, i32, i32, f64, f64, vp, vp, i32, i32, vp, vp, vp]
        assert L.spicey_noise_host_req_bytes() == C.sizeof(abi.SpiceyAcNoiseReq)
        _LIB = L
    return _LIB


class Refused(ValueError):
    pass


def reduce(out_v, out_i, R, freqs, req, n_inst=None, n_freq=None, nR=None, have_out=True, work_bytes=-1):
    """(spec, contrib, total) of the harness for an injected sweep's complex out_v [ni][nf][n_v], out_i [ni][nf][n_i], R
    [ni][nR] and a request abi.ac_noise_req(...).  n_inst, n_freq, nR, have_out, work_bytes: what the call states instead of
    the arrays' own (the refusals).  A refusal raises Refused with the judge's text, after checking that the results kept
    their sentinel."""
    L = lib()
    out_v = np.ascontiguousarray(out_v, dtype=np.complex128)
    out_i = np.ascontiguousarray(out_i, dtype=np.complex128)
    R = np.ascontiguousarray(R, dtype=np.float64)
    freqs = np.ascontiguousarray(freqs, dtype=np.float64)
    ni = out_i.shape[0] if n_inst is None else n_inst
    nf = out_i.shape[1] if n_freq is None else n_freq
    nr = R.shape[1] if nR is None else nR
    spec = np.full((max(ni, 1), max(nf, 1), abi.NOISE_SPEC), SENTINEL)
    contrib = np.full((max(ni, 1), max(nr, 1)), SENTINEL)
    total = np.full((max(ni, 1), 2), SENTINEL)
    err = C.create_string_buffer(256)
    rc = L.spicey_noise_host_run(ni, nf, out_v.ctypes.data, out_v.shape[2], out_i.ctypes.data, out_i.shape[2], R.ctypes.data, nr, freqs.ctypes.data,
                                 C.addressof(req) if req is not None else None, spec.ctypes.data, contrib.ctypes.data, total.ctypes.data, int(have_out),
                                 work_bytes, err, 256)
    if rc != abi.OK:
        assert rc == abi.ERR_BAD_DESC and (spec == SENTINEL).all() and (contrib == SENTINEL).all() and (total == SENTINEL).all()
        raise Refused(err.value.decode())
    return spec, contrib, total


def sweep(flat, freqs, vph, node_p=0, node_n=0, amp=1.0, T=64, resident=False, reverse=False, no_dense=False, stride=3):
    """The AC sweep of `flat` through the host form of ac_exec.h with `amp` injected into node_p and drawn from node_n (both 0:
    no injection); vph None: every phasor zero.  Returns the dict of AcHandle.run plus `slot_status` [n_inst][n_freq], `pos`
    (pivot row and column of node_p, of node_n) and `dense` (solves the fallback repeated)."""
    L = lib()
    d = flat.desc()
    freqs = np.ascontiguousarray(freqs, dtype=np.float64)
    ni, nf = flat.n_inst, len(freqs)
    ph = None
    if vph is not None:
        ph = np.ascontiguousarray(np.broadcast_to(np.asarray(vph, np.complex128).reshape(-1, flat.nV), (ni, flat.nV)))
    out_v = np.zeros((ni, nf, flat.n_out), np.complex128)
    out_i = np.zeros((ni, nf, flat.nR + flat.nC + flat.nL + flat.nV), np.complex128)
    st = np.zeros((ni, nf), np.int32)
    pos = np.zeros(4, np.int32)
    dense = C.c_int32(0)
    a = complex(amp)
    rc = L.spicey_noise_host_sweep(C.byref(d), T, nf, freqs.ctypes.data, ph.ctypes.data if ph is not None else None, node_p, node_n, a.real, a.imag,
                                   out_v.ctypes.data, out_i.ctypes.data, (1 if reverse else 0) | (2 if resident else 0) | (4 if no_dense else 0), stride,
                                   st.ctypes.data, pos.ctypes.data, C.byref(dense))
    bad = st != 0
    inst_status = np.zeros(ni, np.int32)
    first = np.full(ni, -1, np.int64)
    for j in np.nonzero(bad.any(axis=1))[0]:
        first[j] = int(np.argmax(bad[j]))
        inst_status[j] = abi.ERR_SINGULAR if st[j, first[j]] == 1 else abi.ERR_COMPLEX_DIV
    if rc == abi.ERR_SINGULAR and not bad.any():  # (structurally singular: answered without a sweep)
        inst_status[:] = rc
    return {"status": rc, "detail": "" if rc == abi.OK else f"host sweep status {rc}", "out_v": out_v, "out_i": out_i, "slot_status": st,
            "inst_status": inst_status, "first_freq": first, "pos": pos.tolist(), "dense": dense.value}


class HostNoiseBackend:
    """run_ac_noise of a backend on the CPU: the harness's injected sweep, then its reduction.  `launches` lists the
    instance count of every call, like HipBackend.ac_launches."""

    def __init__(self, T=64, resident=False):
        self.T, self.resident = T, resident
        self.launches = []

    def run_ac_noise(self, flat, freqs, node_p, node_n, req):
        self.launches.append(flat.n_inst)
        res = sweep(flat, freqs, None, node_p, node_n, 1.0, T=self.T, resident=self.resident)
        if res["status"] not in (abi.OK, abi.ERR_SINGULAR, abi.ERR_COMPLEX_DIV) or (res["status"] != abi.OK and not res["slot_status"].any()):
            return res
        with np.errstate(all="ignore"):
            res["spec"], res["contrib"], res["total"] = reduce(res["out_v"], res["out_i"], flat.R_val, freqs, req)
        res["gain"] = res["out_i"][:, :, req.in_col] if req.in_col >= 0 else None
        return res


def noise_inputs(n_inst, n_freq, nR, n_extra, n_v, seed):
    """Seeded inputs of the reduction: currents and voltages of both signs over several decades, resistances that differ per
    instance, ascending frequencies of uneven spacing."""
    rng = np.random.default_rng(seed)
    n_i = nR + n_extra

    def cx(shape):
        mag = 10.0 ** rng.uniform(-6, 1, shape)
        return mag * np.exp(1j * rng.uniform(0, 2 * np.pi, shape))
    out_i, out_v = cx((n_inst, n_freq, n_i)), cx((n_inst, n_freq, n_v))
    R = 10.0 ** rng.uniform(0, 6, (n_inst, nR)) * (1.0 + 0.37 * np.arange(n_inst))[:, None]
    freqs = np.cumsum(10.0 ** rng.uniform(0, 5, n_freq))
    return out_v, out_i, R, freqs


def bits_equal(a, b):
    a = np.ascontiguousarray(a, dtype=np.float64)
    b = np.ascontiguousarray(b, dtype=np.float64)
    return (a.view(np.int64) == b.view(np.int64)) | (np.isnan(a) & np.isnan(b))
