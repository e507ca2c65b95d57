"""ctypes view of the CPU harness of the waveform measurements (tests/measure_host/harness.cpp) and the request lists the
host and GPU tests share."""
import ctypes as C
import os

import numpy as np

import harness_build
from spicey_amd import abi
from spicey_amd.measure import make_reqs, reduce_reference

HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None


def lib():
    global _LIB
    if _LIB is None:
        L = harness_build.load(HERE, "libspicey_measure_host.so")
        L.spicey_meas_host_chunk.restype = C.c_int32
        L.spicey_meas_host_threads.restype = C.c_int32
        L.spicey_meas_host_workspace_bytes.restype = C.c_int64
        L.spicey_meas_host_workspace_bytes.argtypes = [C.c_int32, C.c_int64, C.c_int32]
        L.spicey_meas_host_run.restype = C.c_int32
        L.spicey_meas_host_run.argtypes = [C.c_int32, C.c_int64, C.c_double, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32,
                                           C.c_void_p, C.c_int32, C.c_int64, C.c_char_p, C.c_int32]
        _LIB = L
    return _LIB


def chunk() -> int:
    return lib().spicey_meas_host_chunk()


class Refused(ValueError):
    pass


def run(out_v, out_i, reqs, dt, threads=None, grid=0):
    """meas [n_inst][n_req][8] of the harness; threads / grid: the emulated launch (default: the kernels' own)."""
    L = lib()
    out_v = np.ascontiguousarray(out_v, dtype=np.float64)
    out_i = np.ascontiguousarray(out_i, dtype=np.float64) if out_i is not None else None
    r = np.ascontiguousarray(reqs, dtype=abi.MEAS_REQ_DTYPE).reshape(-1)
    ni, n_points, n_v = out_v.shape
    meas = np.full((ni, max(len(r), 1), 8), np.nan)
    err = C.create_string_buffer(256)
    rc = L.spicey_meas_host_run(ni, n_points, dt, out_v.ctypes.data, n_v, out_i.ctypes.data if out_i is not None else None,
                                out_i.shape[2] if out_i is not None else 0, r.ctypes.data if len(r) else None, len(r), meas.ctypes.data,
                                threads or L.spicey_meas_host_threads(), grid, err, 256)
    if rc != abi.OK:
        raise Refused(err.value.decode())
    return meas[:, :len(r)]


def waveforms(n_inst, n_points, n_v, n_i, seed):
    """Seeded samples, most of them from nine values a quarter apart — equal extremes (first-occurrence ties) and samples
    exactly on a level occur all the time — the rest continuous, so the sums round."""
    rng = np.random.default_rng(seed)

    def one(n):
        q = rng.integers(-4, 5, size=(n_inst, n_points, n)) / 4.0
        c = rng.uniform(-0.99, 0.99, size=(n_inst, n_points, n))
        return np.ascontiguousarray(np.where(rng.random((n_inst, n_points, n)) < 0.7, q, c))
    return one(n_v), one(n_i)


def windows(n_points):
    """(from, to) pairs: the whole run (to = -1 and explicit), single points, and windows that start and end in the middle
    of a chunk and on chunk edges."""
    c = chunk()
    marks = sorted({s for s in (0, 1, 37, c - 1, c, c + 1, c + 100, 2 * c - 1, 2 * c, 2 * c + 1, 3 * c, n_points // 2, n_points - 2, n_points - 1)
                    if 0 <= s < n_points})
    out = [(0, -1), (0, n_points - 1)]
    out += [(s, s) for s in marks]
    out += [(a, b) for a in marks for b in marks if a < b]
    return out


def request_pool(n_points, n_v, n_i, count, seed):
    """`count` requests cycling through the windows, both kinds and signals, all three directions, columns with and without
    a reference column; every fifth one repeats an earlier request."""
    rng = np.random.default_rng(seed)
    wins = windows(n_points)
    rows = []
    for k in range(count):
        if k % 5 == 4:
            rows.append(rows[int(rng.integers(0, len(rows)))])
            continue
        a, b = wins[k % len(wins)]
        sig = (k // 6) % 2
        n = n_i if sig else n_v
        col = (k * 7 + k // 3) % n
        col_ref = int(rng.integers(0, n)) if k % 3 == 2 else -1
        if k % 2 == 0:
            rows.append((abi.MEAS_STATS, sig, col, col_ref, a, b, 0.0, 0))
        else:
            rows.append((abi.MEAS_CROSS, sig, col, col_ref, a, b, (0.25, 0.1, -0.5, 0.0)[(k // 2) % 4], (1, -1, 0)[(k // 2) % 3]))
    return make_reqs(rows)


U = 2.0 ** -52


def bits_equal(a, b):
    a = np.ascontiguousarray(a, dtype=np.float64)
    b = np.ascontiguousarray(b, dtype=np.float64)
    return (a.view(np.int64) == b.view(np.int64)) | (np.isnan(a) & np.isnan(b))


def signal_of(out_v, out_i, q):
    """The samples of request q's window, [n_inst][n]."""
    a = out_i if int(q["signal"]) else out_v
    s1 = a.shape[1] - 1 if int(q["step_to"]) == -1 else int(q["step_to"])
    x = a[:, int(q["step_from"]):s1 + 1, int(q["col"])]
    if int(q["col_ref"]) >= 0:
        x = x - a[:, int(q["step_from"]):s1 + 1, int(q["col_ref"])]
    return x


def check_against_reference(got, out_v, out_i, reqs, dt, rows=None):
    """The rules of every comparison with reduce_reference, on the CPU and on the GPU: crossings and the order-free fields
    of stats (min, max, their steps, first, last) bit for bit; sum within n 2^-52 sum |x| and sumsq within (n + 1) 2^-52
    sum x^2 of the exactly rounded sums — the bound of any summation order (n - 1 additions, each of relative error
    2^-53, compound to less than n 2^-53; the squares add one rounding each; the factor 2 is slack for the bound's own
    evaluation).  rows: the instances to look at (default all)."""
    import math
    ref = reduce_reference(out_v, out_i, reqs, dt)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    rows = range(got.shape[0]) if rows is None else rows
    for r, q in enumerate(reqs):
        for i in rows:
            if int(q["kind"]) == abi.MEAS_CROSS:
                assert bits_equal(got[i, r], ref[i, r]).all(), (i, r, q, got[i, r], ref[i, r])
                continue
            free = [0, 1, 2, 3, 6, 7]
            assert bits_equal(got[i, r][free], ref[i, r][free]).all(), (i, r, q, got[i, r], ref[i, r])
            xs = signal_of(out_v, out_i, q)[i].tolist()
            n = len(xs)
            exact_s, abs_s = math.fsum(xs), math.fsum(abs(v) for v in xs)
            exact_q = math.fsum(v * v for v in xs)
            for val in (got[i, r, 4], ref[i, r, 4]):
                assert abs(val - exact_s) <= n * U * abs_s, (i, r, val, exact_s)
            for val in (got[i, r, 5], ref[i, r, 5]):
                assert abs(val - exact_q) <= (n + 1) * U * exact_q, (i, r, val, exact_q)
