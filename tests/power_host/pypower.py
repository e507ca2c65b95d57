"""ctypes view of the CPU harness of the products of two signals (tests/power_host/harness.cpp) and the request lists the
host and GPU tests share."""
import ctypes as C
import math
import os

import numpy as np

import harness_build
from spicey_amd import abi
from spicey_amd.measure import make_power_reqs, reduce_reference_power

HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None

FREE = [0, 1, 2, 3, 5, 6, 9, 10, 11, 12]  # the order-free fields of a row
SUMS = [4, 7, 8]                           # sum_p, sum_aa, sum_bb
U = 2.0 ** -52


def lib():
    global _LIB
    if _LIB is None:
        L = harness_build.load(HERE, "libspicey_power_host.so")
        L.spicey_power_host_chunk.restype = C.c_int32
        L.spicey_power_host_threads.restype = C.c_int32
        L.spicey_power_host_workspace_bytes.restype = C.c_int64
        L.spicey_power_host_workspace_bytes.argtypes = [C.c_int32, C.c_int64, C.c_int32]
        L.spicey_power_host_run.restype = C.c_int32
        L.spicey_power_host_run.argtypes = [C.c_int32, C.c_int64, C.c_double, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32,
                                            C.c_void_p, C.c_int32, C.c_int64, C.c_int32, C.c_int64, C.c_char_p, C.c_int32]
        _LIB = L
    return _LIB


def chunk() -> int:
    return lib().spicey_power_host_chunk()


class Refused(ValueError):
    pass


SENTINEL = -7.25


def run(out_v, out_i, reqs, dt, threads=None, grid=0, n_inst=None, n_points=None, have_out=True, work_bytes=-1):
    """rows [n_inst][n_req][16] of the harness; threads / grid: the emulated launch (default: the kernels' own).  n_inst,
    n_points, have_out, work_bytes: what the call states instead of the arrays' own (the refusals).  A refusal raises Refused
    with the judge's text, after checking that the result array kept its sentinel."""
    L = lib()
    out_v = np.ascontiguousarray(out_v, dtype=np.float64) if out_v is not None else None
    out_i = np.ascontiguousarray(out_i, dtype=np.float64) if out_i is not None else None
    r = np.ascontiguousarray(reqs, dtype=abi.POWER_REQ_DTYPE).reshape(-1)
    shape = (out_v if out_v is not None else out_i).shape
    ni = shape[0] if n_inst is None else n_inst
    npts = shape[1] if n_points is None else n_points
    rows = np.full((max(ni, 1), max(len(r), 1), abi.POWER_ROW), SENTINEL)
    err = C.create_string_buffer(256)
    rc = L.spicey_power_host_run(ni, npts, dt, out_v.ctypes.data if out_v is not None else None, out_v.shape[2] if out_v is not None else 0,
                                 out_i.ctypes.data if out_i is not None else None, out_i.shape[2] if out_i is not None else 0,
                                 r.ctypes.data if len(r) else None, len(r), rows.ctypes.data, int(have_out), work_bytes,
                                 threads or L.spicey_power_host_threads(), grid, err, 256)
    if rc != abi.OK:
        assert rc == abi.ERR_BAD_DESC and (rows == SENTINEL).all()
        raise Refused(err.value.decode())
    return rows[:, :len(r)]


def waveforms(n_inst, n_points, n_v, n_i, seed):
    """Seeded samples, most of them from nine values a quarter apart — equal products (first-occurrence ties) occur all the
    time — the rest continuous, so the products and sums round."""
    rng = np.random.default_rng(seed)

    def one(n):
        q = rng.integers(-4, 5, size=(n_inst, n_points, n)) / 4.0
        c = rng.uniform(-0.99, 0.99, size=(n_inst, n_points, n))
        return np.ascontiguousarray(np.where(rng.random((n_inst, n_points, n)) < 0.7, q, c))
    return one(n_v), one(n_i)


def combination(k):
    """(a_signal, b_signal, a_col_ref present, b_col_ref present, neg) of request k: the bits of k mod 32."""
    m = k % 32
    return m & 1, (m >> 1) & 1, bool((m >> 2) & 1), bool((m >> 3) & 1), (m >> 4) & 1


def request_pool(n_points, n_v, n_i, count, seed):
    """`count` requests, request k with combination(k): random columns, a reference column different from the column where
    the array has two (else the column itself: a factor of exact zeros); windows in turn the whole run, one sample, and
    random sub-windows (they start anywhere in a chunk); from the third round on every fifth request repeats an earlier one
    of its own combination."""
    rng = np.random.default_rng(seed)
    rows = []
    for k in range(count):
        if k >= 64 and k % 5 == 4:
            rows.append(rows[k - 32 * int(rng.integers(1, k // 32 + 1))])
            continue
        sa, sb, ra, rb, neg = combination(k)

        def cols(sig, ref):
            n = n_i if sig else n_v
            col = int(rng.integers(0, n))
            if not ref:
                return col, -1
            return col, (col + 1 + int(rng.integers(0, n - 1))) % n if n > 1 else col

        ca, cra = cols(sa, ra)
        cb, crb = cols(sb, rb)
        w = (k // 32 + k) % 4
        if w == 0:
            s0, s1 = 0, (-1 if k % 2 else n_points - 1)
        elif w == 1:
            s0 = s1 = int(rng.integers(0, n_points))
        else:
            s0 = int(rng.integers(0, n_points))
            s1 = int(rng.integers(s0, n_points))
        rows.append((sa, ca, cra, sb, cb, crb, neg, s0, s1))
    return make_power_reqs(rows)


def bits_equal(a, b):
    a = np.ascontiguousarray(a, dtype=np.float64)
    b = np.ascontiguousarray(b, dtype=np.float64)
    return (a.view(np.int64) == b.view(np.int64)) | (np.isnan(a) & np.isnan(b))


def factor_of(out_v, out_i, q, pre):
    """The samples of factor `pre` ("a_" / "b_") over request q's window, [n_inst][n]."""
    a = out_i if int(q[pre + "signal"]) else out_v
    s1 = a.shape[1] - 1 if int(q["step_to"]) == -1 else int(q["step_to"])
    x = a[:, int(q["step_from"]):s1 + 1, int(q[pre + "col"])]
    if int(q[pre + "col_ref"]) >= 0:
        x = x - a[:, int(q["step_from"]):s1 + 1, int(q[pre + "col_ref"])]
    return x


def check_against_reference(got, out_v, out_i, reqs, dt, rows=None):
    """The rules of every comparison with reduce_reference_power, on the CPU and on the GPU: the ten order-free fields (the
    extremes, their steps, first and last of p, a and b) bit for bit, the tail of the row 0, and sum_p, sum_aa, sum_bb
    within (n + 1) 2^-52 sum |term| of the exactly rounded sum of the terms — the bound of any summation order: n - 1
    additions, each of relative error 2^-53, compound to less than n 2^-53, the products add one rounding each, and the
    factor 2 is slack for the bound's own evaluation.  rows: the instances to look at (default all)."""
    ref = reduce_reference_power(out_v, out_i, reqs, dt)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    rows = range(got.shape[0]) if rows is None else rows
    for r, q in enumerate(reqs):
        a, b = factor_of(out_v, out_i, q, "a_"), factor_of(out_v, out_i, q, "b_")
        p = -(a * b) if int(q["neg"]) else a * b
        for i in rows:
            assert bits_equal(got[i, r][FREE], ref[i, r][FREE]).all(), (i, r, q, got[i, r], ref[i, r])
            assert (got[i, r, 13:] == 0.0).all() and (ref[i, r, 13:] == 0.0).all(), (i, r)
            n = p.shape[1]
            for j, terms in zip(SUMS, (p[i].tolist(), (a[i] * a[i]).tolist(), (b[i] * b[i]).tolist())):
                exact, mag = math.fsum(terms), math.fsum(abs(t) for t in terms)
                for val in (got[i, r, j], ref[i, r, j]):
                    assert abs(val - exact) <= (n + 1) * U * mag, (i, r, j, val, exact)
