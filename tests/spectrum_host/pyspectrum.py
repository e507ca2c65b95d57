"""ctypes view of the CPU harness of the spectrum pass (tests/spectrum_host/harness.cpp), the waveforms and request lists
the host and GPU tests share, and the one checker of every comparison with a long-double DFT."""
import ctypes as C
import math
import os

import numpy as np

import harness_build
from spicey_amd import abi
from spicey_amd.measure import make_spec_reqs

HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None

N_INST, N_I, DT = 3, 5, 1e-6
N_VS = (1, 5, 65)
# the N/2 butterflies of a stage: below one wave, one wave, the workgroup, more than the workgroup
LOG2NS = (3, 6, 7, 8, 9, 10, 11)


def lib():
    global _LIB
    if _LIB is None:
        L = harness_build.load(HERE, "libspicey_spectrum_host.so")
        L.spicey_spec_host_threads.restype = C.c_int32
        L.spicey_spec_host_workspace_bytes.restype = C.c_int64
        L.spicey_spec_host_workspace_bytes.argtypes = [C.c_int32, C.c_int64, C.c_void_p, C.c_int32]
        L.spicey_spec_host_lds_bytes.restype = C.c_int64
        L.spicey_spec_host_lds_bytes.argtypes = [C.c_int32]
        L.spicey_spec_host_tables.restype = None
        L.spicey_spec_host_tables.argtypes = [C.c_int32, C.c_void_p, C.c_void_p]
        L.spicey_spec_host_run.restype = C.c_int32
        L.spicey_spec_host_run.argtypes = [C.c_int32, C.c_int64, C.c_double, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32,
                                           C.c_void_p, C.c_int32, C.c_int64, C.c_int32, C.c_int64, C.c_char_p, C.c_int32]
        _LIB = L
    return _LIB


class Refused(ValueError):
    pass


def _r(reqs):
    return np.ascontiguousarray(reqs, dtype=abi.SPEC_REQ_DTYPE).reshape(-1)


def width(reqs) -> int:
    return abi.spec_row_doubles(reqs)


def own_width(q) -> int:
    return 2 * (int(q["bin_to"]) - int(q["bin_from"]) + 1) if int(q["kind"]) == abi.SPEC_BINS else abi.SPEC_DOM_DOUBLES


def workspace_bytes(n_inst, n_points, reqs) -> int:
    r = _r(reqs)
    return lib().spicey_spec_host_workspace_bytes(n_inst, n_points, r.ctypes.data if len(r) else None, len(r))


def lds_bytes(log2n) -> int:
    return lib().spicey_spec_host_lds_bytes(log2n)


def tables(log2n):
    """(T [N/2] complex, w [N]) as the library uploads them."""
    N = 1 << log2n
    T, w = np.zeros(N), np.zeros(N)
    lib().spicey_spec_host_tables(log2n, T.ctypes.data, w.ctypes.data)
    return T[0::2] + 1j * T[1::2], w


def run(out_v, out_i, reqs, dt=DT, threads=None, grid=0, out_stride=None, work_bytes=-1, fill=np.nan):
    """Rows [n_inst][n_req][out_stride] of the harness (out_stride: default the longest request's row); threads / grid: the
    emulated launch (default: the kernel's own).  A refusal raises Refused with the result buffer still holding `fill`."""
    L = lib()
    out_v = np.ascontiguousarray(out_v, dtype=np.float64)
    out_i = np.ascontiguousarray(out_i, dtype=np.float64) if out_i is not None else None
    r = _r(reqs)
    ni, n_points, n_v = out_v.shape
    stride = width(r) if out_stride is None else out_stride
    out = np.full((ni, max(len(r), 1), max(stride, 1)), fill)
    err = C.create_string_buffer(256)
    rc = L.spicey_spec_host_run(ni, n_points, dt, out_v.ctypes.data, n_v, out_i.ctypes.data if out_i is not None else None,
                                out_i.shape[2] if out_i is not None else 0, r.ctypes.data if len(r) else None, len(r), out.ctypes.data, stride,
                                work_bytes, threads or L.spicey_spec_host_threads(), grid, err, 256)
    if rc != abi.OK:
        assert rc == abi.ERR_BAD_DESC and bits_equal(out, np.full_like(out, fill)).all()
        raise Refused(err.value.decode())
    return out[:, :len(r)]


def bits_equal(a, b):
    a = np.ascontiguousarray(a, dtype=np.float64)
    b = np.ascontiguousarray(b, dtype=np.float64)
    return (a.view(np.int64) == b.view(np.int64)) | (np.isnan(a) & np.isnan(b))


def waveforms(n_inst, n_points, n_v, n_i, seed):
    """Seeded samples: Gaussian columns, and on every third column an off-bin tone with an offset."""
    rng = np.random.default_rng(seed)

    def one(n):
        a = rng.standard_normal((n_inst, n_points, n))
        s = np.arange(n_points)[None, :, None]
        tone = 0.75 + 1.5 * np.sin(2.0 * np.pi * (0.0371 + 0.001 * np.arange(n)[None, None, :]) * s + np.arange(n_inst)[:, None, None])
        return np.ascontiguousarray(np.where((np.arange(n) % 3 == 2)[None, None, :], tone, a))
    return one(n_v), one(n_i)


def bands(log2n):
    """The full band, DC alone, Nyquist alone, a single inner bin."""
    half = (1 << log2n) // 2
    return [(0, half), (0, 0), (half, half), (half // 2 + 1, half // 2 + 1)]


def request_pool(n_points, n_v, n_i, seed, log2ns=LOG2NS):
    """Requests over every N of `log2ns` that fits the run: first steps 0, 3 and the run's last N samples, the four bands,
    both windows, both kinds, both signals, columns with and without a reference column; after every fourth one an earlier
    request is repeated."""
    rng = np.random.default_rng(seed)
    rows = []
    k = 0
    for log2n in log2ns:
        N = 1 << log2n
        for s0 in sorted({s for s in (0, 3, n_points - N) if 0 <= s <= n_points - N}):
            for b0, b1 in bands(log2n):
                sig = (k // 3) % 2
                n = n_i if sig else n_v
                col = (k * 7 + k // 3) % n
                col_ref = int(rng.integers(0, n)) if k % 3 == 2 else -1
                rows.append((sig, col, col_ref, (k // 2) % 2, s0, log2n, k % 2, b0, b1))
                k += 1
                if k % 4 == 0:
                    rows.append(rows[int(rng.integers(0, len(rows)))])
    order = rng.permutation(len(rows))  # (the lengths mixed, not in ascending groups)
    return make_spec_reqs([rows[i] for i in order])


def samples_of(out_v, out_i, q):
    """The N samples of request q, [n_inst][N] (the subtraction included)."""
    a = out_i if int(q["signal"]) else out_v
    s0, N = int(q["step_from"]), 1 << int(q["log2n"])
    x = a[:, s0:s0 + N, int(q["col"])]
    if int(q["col_ref"]) >= 0:
        x = x - a[:, s0:s0 + N, int(q["col_ref"])]
    return x


LD = np.longdouble
U = 2.0 ** -53


def _ld_unit_circle(N):
    """exp(-2 pi i m / N), m = 0 .. N-1, in long double, as (cos, -sin)."""
    a = (8 * np.arctan(LD(1))) * np.arange(N, dtype=LD) / LD(N)
    return np.cos(a), -np.sin(a)


def twiddle_error(log2n) -> float:
    """mu: the largest distance of an uploaded twiddle from the long-double value."""
    N = 1 << log2n
    T, _ = tables(log2n)
    c, s = _ld_unit_circle(N)
    return float(np.max(np.hypot(T.real.astype(LD) - c[:N // 2], T.imag.astype(LD) - s[:N // 2])))


def dft_bound(log2n, y_norm2, mu) -> float:
    """Higham, Accuracy and Stability of Numerical Algorithms, Thm 24.2, for the radix-2 FFT of N = 2^t points with
    twiddles in error by at most mu: ||err||_2 <= t eta / (1 - t eta) ||X||_2, eta = mu + gamma_4 (sqrt 2 + mu), gamma_4 =
    4 u / (1 - 4 u), u = 2^-53; with ||X||_2 = sqrt N ||y||_2 it bounds every bin: |err_k| <= t eta / (1 - t eta) sqrt N
    ||y||_2."""
    g4 = 4 * U / (1 - 4 * U)
    eta = mu + g4 * (math.sqrt(2.0) + mu)
    t = log2n
    return t * eta / (1 - t * eta) * math.sqrt(1 << log2n) * y_norm2


def dft_bins(y, ks):
    """Bins `ks` of the direct DFT of the rows of y [n][N] in long double: (re, im) [n][len(ks)]."""
    N = y.shape[1]
    c, s = _ld_unit_circle(N)
    idx = (np.arange(N, dtype=np.int64)[:, None] * np.asarray(ks, dtype=np.int64)[None, :]) % N
    yl = y.astype(LD)
    return yl @ c[idx], yl @ s[idx]


def check_against_dft(got, out_v, out_i, reqs, max_log2n=10, bins=None, seed=0):
    """Every kind 0 bin (or `bins` seeded ones per request) and every dominant's (re_k, im_k) of `got` against the direct
    long-double DFT of the same double-rounded windowed samples, under dft_bound with the measured mu.  Requests longer than
    2^max_log2n are skipped.  Returns the largest error seen as a fraction of its bound."""
    reqs = _r(reqs)
    rng = np.random.default_rng(seed)
    worst = 0.0
    for r, q in enumerate(reqs):
        log2n = int(q["log2n"])
        if log2n > max_log2n:
            continue
        x = samples_of(out_v, out_i, q)
        y = x * tables(log2n)[1][None, :] if int(q["window"]) == abi.SPEC_HANN else x
        mu = twiddle_error(log2n)
        norms = np.sqrt(np.sum(y.astype(LD) ** 2, axis=1)).astype(np.float64)
        if int(q["kind"]) == abi.SPEC_BINS:
            ks = np.arange(int(q["bin_from"]), int(q["bin_to"]) + 1)
            cols = np.arange(len(ks))
            if bins is not None and len(ks) > bins:
                cols = np.sort(rng.choice(len(ks), bins, replace=False))
            re, im = dft_bins(y, ks[cols])
            g_re, g_im = got[:, r, 2 * cols], got[:, r, 2 * cols + 1]
        else:
            rows = [i for i in range(got.shape[0]) if got[i, r, 0] >= 0]
            if not rows:
                continue
            g_re, g_im = np.zeros((got.shape[0], 1)), np.zeros((got.shape[0], 1))
            re, im = np.zeros((got.shape[0], 1), LD), np.zeros((got.shape[0], 1), LD)
            for i in rows:
                a, b = dft_bins(y[i:i + 1], [int(got[i, r, 0])])
                re[i], im[i], g_re[i], g_im[i] = a[0], b[0], got[i, r, 1], got[i, r, 2]
        err = np.hypot(g_re.astype(LD) - re, g_im.astype(LD) - im).astype(np.float64)
        for i in range(got.shape[0]):
            bound = dft_bound(log2n, float(norms[i]), mu)
            assert (err[i] <= bound).all(), (i, r, q, err[i].max(), bound)
            if bound > 0:
                worst = max(worst, float(err[i].max()) / bound)
    return worst
