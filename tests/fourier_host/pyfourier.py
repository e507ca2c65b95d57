"""ctypes view of the CPU harness of the harmonics pass (tests/fourier_host/harness.cpp), the request lists the host and
GPU tests share, and the one checker of every comparison with reduce_reference_fourier."""
import ctypes as C
import math
import os

import numpy as np

import harness_build
from spicey_amd import abi
from spicey_amd.measure import make_four_reqs, reduce_reference_fourier

HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None


def lib():
    global _LIB
    if _LIB is None:
        L = harness_build.load(HERE, "libspicey_fourier_host.so")
        for fn in ("chunk", "threads", "max_harm"):
            getattr(L, "spicey_four_host_" + fn).restype = C.c_int32
        L.spicey_four_host_workspace_bytes.restype = C.c_int64
        L.spicey_four_host_workspace_bytes.argtypes = [C.c_int32, C.c_int64, C.c_void_p, C.c_int32]
        L.spicey_four_host_twiddle.restype = None
        L.spicey_four_host_twiddle.argtypes = [C.c_int32, C.c_int64, C.c_double, C.c_void_p]
        L.spicey_four_host_run.restype = C.c_int32
        L.spicey_four_host_run.argtypes = [C.c_int32, C.c_int64, C.c_double, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32,
                                           C.c_void_p, C.c_int32, C.c_int64, C.c_int32, C.c_int64, C.c_char_p, C.c_int32]
        _LIB = L
    return _LIB


def chunk() -> int:
    return lib().spicey_four_host_chunk()


class Refused(ValueError):
    pass


def _r(reqs):
    return np.ascontiguousarray(reqs, dtype=abi.FOUR_REQ_DTYPE).reshape(-1)


def width(reqs) -> int:
    r = _r(reqs)
    return 1 + 2 * int(r["n_harm"].max()) if len(r) else 1


def workspace_bytes(n_inst, n_points, reqs) -> int:
    r = _r(reqs)
    return lib().spicey_four_host_workspace_bytes(n_inst, n_points, r.ctypes.data if len(r) else None, len(r))


def run(out_v, out_i, reqs, dt, threads=None, grid=0, out_stride=None, work_bytes=-1, fill=np.nan):
    """Rows [n_inst][n_req][out_stride] of the harness (out_stride: default 1 + 2 max n_harm); threads / grid: the emulated
    launch (default: the kernels' own).  A refusal raises Refused with the result buffer still holding `fill`."""
    L = lib()
    out_v = np.ascontiguousarray(out_v, dtype=np.float64)
    out_i = np.ascontiguousarray(out_i, dtype=np.float64) if out_i is not None else None
    r = _r(reqs)
    ni, n_points, n_v = out_v.shape
    stride = width(r) if out_stride is None else out_stride
    out = np.full((ni, max(len(r), 1), max(stride, 1)), fill)
    err = C.create_string_buffer(256)
    rc = L.spicey_four_host_run(ni, n_points, dt, out_v.ctypes.data, n_v, out_i.ctypes.data if out_i is not None else None,
                                out_i.shape[2] if out_i is not None else 0, r.ctypes.data if len(r) else None, len(r), out.ctypes.data, stride,
                                work_bytes, threads or L.spicey_four_host_threads(), grid, err, 256)
    if rc != abi.OK:
        assert rc == abi.ERR_BAD_DESC and bits_equal(out, np.full_like(out, fill)).all()
        raise Refused(err.value.decode())
    return out[:, :len(r)]


def twiddle(h, s, f0dt):
    """(c, s) of the library's host function."""
    cs = np.zeros(2)
    lib().spicey_four_host_twiddle(h, s, f0dt, cs.ctypes.data)
    return float(cs[0]), float(cs[1])


def bases(n_points, dt):
    """(f0, step_from, step_to) triples of different lengths: the whole run, windows on and off chunk edges, one sample.
    f0 keeps 16 harmonics under Nyquist."""
    c = chunk()
    last = n_points - 1
    f = 1.0 / (40.0 * dt)
    cand = [(f, 0, -1), (f, 0, last), (f * 0.77, 1, last), (f, last - 1, last), (f * 1.1, 0, 1),
            (f, c, 2 * c), (f, c - 1, 2 * c + 1), (f * 0.5, c + 1, 3 * c), (f, 37, c + 100), (f, 2 * c, last), (f * 0.31, 0, c), (f, c, c + 1), (f * 0.9, 0, last)]
    out = []
    for f0, a, b in cand:
        bb = last if b == -1 else b
        if 0 <= a < bb <= last and (f0, a, b) not in out:
            out.append((f0, a, b))
    return out


def request_pool(n_points, n_v, n_i, count, dt, seed, n_harm=(1, 9, 16)):
    """`count` requests cycling through the bases, both signals, columns with and without a reference column and the
    harmonic counts; every fifth one repeats an earlier request."""
    rng = np.random.default_rng(seed)
    bs = bases(n_points, dt)
    rows = []
    for k in range(count):
        if k % 5 == 4 and rows:
            rows.append(rows[int(rng.integers(0, len(rows)))])
            continue
        f0, a, b = bs[k % len(bs)]
        sig = (k // 6) % 2
        n = n_i if sig else n_v
        col = (k * 7 + k // 3) % n
        col_ref = int(rng.integers(0, n)) if k % 3 == 2 else -1
        rows.append((sig, col, col_ref, n_harm[(k // 2) % len(n_harm)], a, b, f0))
    return make_four_reqs(rows)


U = 2.0 ** -52


def bits_equal(a, b):
    a = np.ascontiguousarray(a, dtype=np.float64)
    b = np.ascontiguousarray(b, dtype=np.float64)
    return (a.view(np.int64) == b.view(np.int64)) | (np.isnan(a) & np.isnan(b))


def signal_of(out_v, out_i, q):
    """The samples of request q's window step_from .. step_to - 1, [n_inst][N]."""
    a = out_i if int(q["signal"]) else out_v
    s1 = a.shape[1] - 1 if int(q["step_to"]) == -1 else int(q["step_to"])
    x = a[:, int(q["step_from"]):s1, int(q["col"])]
    if int(q["col_ref"]) >= 0:
        x = x - a[:, int(q["step_from"]):s1, int(q["col_ref"])]
    return x


def check_against_reference(got, out_v, out_i, reqs, dt, rows=None):
    """The rule of every comparison with reduce_reference_fourier, on the CPU and on the GPU.  With n = the window's
    samples and u = 2^-53 (one rounding):
      C0   |got - ref| <= n 2^-52 sum |x_s|.  Both sides add the same n numbers, in different groupings: n - 1 additions of
           relative error u each compound to at most (n - 1) u (1 + O(n u)) sum |x| on either side — gamma_{n-1} of Higham
           — so 2 (n - 1) u < n 2^-52 between them.
      C_h, S_h   |got - ref| <= (n + 8) 2^-52 sum |x_s|.  Each side: the products x_s t add one rounding each, (1 + u) on
           terms of size <= |x_s| since |t| <= 1 — n u in place of (n - 1) u; and the two sides may hold twiddles from
           different libms, allowed 4 ulp of 1 apart: 4 * 2^-52 sum |x| = 8 u sum |x|.  2 n u + 8 u = (n + 4) 2^-52 <=
           (n + 8) 2^-52; the rest is slack for the bound's own evaluation.
    Elements behind a request's 1 + 2 n_harm must be +0.0.  rows: the instances to look at (default all).  Returns the
    largest distance, in ulps of 1 (2^-52), seen between this libm's twiddles and numpy's over the sampled (h, s) pairs."""
    reqs = _r(reqs)
    ref = reduce_reference_fourier(out_v, out_i, reqs, dt)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    rows = range(got.shape[0]) if rows is None else rows
    worst = 0.0
    for r, q in enumerate(reqs):
        H = int(q["n_harm"])
        xs = signal_of(out_v, out_i, q)
        n = xs.shape[1]
        for i in rows:
            abs_s = math.fsum(abs(v) for v in xs[i].tolist())
            g, e = got[i, r], ref[i, r]
            assert abs(g[0] - e[0]) <= n * U * abs_s, (i, r, q, g[0], e[0])
            d = np.abs(g[1:1 + 2 * H] - e[1:1 + 2 * H])
            assert (d <= (n + 8) * U * abs_s).all(), (i, r, q, d.max(), (n + 8) * U * abs_s)
            assert (g[1 + 2 * H:].view(np.int64) == 0).all(), (i, r, q)
        # this libm against numpy's on the window's first, middle and last step
        f0dt = float(q["f0"]) * dt
        s0 = int(q["step_from"])
        for s in (s0, s0 + n // 2, s0 + n - 1):
            for h in (1, H):
                t = float(h * s) * f0dt
                t = t - math.floor(t)
                a = (2.0 * np.pi) * t
                c, sn = twiddle(h, s, f0dt)
                worst = max(worst, abs(c - float(np.cos(a))) / U, abs(sn - float(np.sin(a))) / U)
    return worst
