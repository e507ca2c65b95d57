"""ctypes view of the CPU harness of the values pass (tests/values_host/harness.cpp) and the inputs and request lists the
host and GPU tests share."""
import ctypes as C
import os

import numpy as np

import harness_build
from spicey_amd import abi
from spicey_amd.measure import make_timing_reqs, make_value_points, make_value_reqs, reduce_reference_timing, reduce_reference_values

HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None


def lib():
    global _LIB
    if _LIB is None:
        L = harness_build.load(HERE, "libspicey_values_host.so")
        for fn in ("chunk", "threads", "max_buckets"):
            getattr(L, "spicey_values_host_" + fn).restype = C.c_int32
        L.spicey_values_host_workspace_bytes.restype = C.c_int64
        L.spicey_values_host_workspace_bytes.argtypes = [C.c_int32, C.c_int64, C.c_void_p, C.c_int32, C.c_int64]
        L.spicey_values_host_run.restype = C.c_int32
        L.spicey_values_host_run.argtypes = [C.c_int32, C.c_int64, C.c_double, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32,
                                             C.c_void_p, C.c_int64, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_int64, C.c_int32, C.c_int64,
                                             C.c_char_p, C.c_int32]
        _LIB = L
    return _LIB


def chunk() -> int:
    return lib().spicey_values_host_chunk()


def workspace_bytes(n_inst, n_points, reqs, n_pts=0) -> int:
    r = np.ascontiguousarray(reqs, dtype=abi.VAL_REQ_DTYPE).reshape(-1)
    return lib().spicey_values_host_workspace_bytes(n_inst, n_points, r.ctypes.data if len(r) else None, len(r), n_pts)


class Refused(ValueError):
    pass


SENTINEL = -7.25


def run(out_v, out_i, reqs, pts, dt, timing=None, threads=None, grid=0, n_inst=None, n_points=None, have_out=True, work_bytes=-1, out_stride=None,
        n_timing=None, n_pts=None):
    """rows [n_inst][n_req][out_stride] of the harness (out_stride: by default the longest request's row); threads / grid:
    the emulated launch (default: the kernels' own).  n_inst, n_points, have_out, work_bytes, n_timing, n_pts: what the call
    states instead of the arrays' own (the refusals).  A refusal raises Refused with the judge's text, after checking that
    the result array kept its sentinel."""
    L = lib()
    out_v = np.ascontiguousarray(out_v, dtype=np.float64) if out_v is not None else None
    out_i = np.ascontiguousarray(out_i, dtype=np.float64) if out_i is not None else None
    timing = np.ascontiguousarray(timing, dtype=np.float64) if timing is not None else None
    r = np.ascontiguousarray(reqs, dtype=abi.VAL_REQ_DTYPE).reshape(-1)
    pt = np.ascontiguousarray(pts, dtype=abi.VAL_POINT_DTYPE).reshape(-1)
    shape = (out_v if out_v is not None else out_i).shape
    ni = shape[0] if n_inst is None else n_inst
    npts = shape[1] if n_points is None else n_points
    stride = abi.val_row_doubles(r) if out_stride is None else out_stride
    rows = np.full((max(ni, 1), max(len(r), 1), max(stride, 1)), SENTINEL)
    err = C.create_string_buffer(256)
    rc = L.spicey_values_host_run(ni, npts, dt, out_v.ctypes.data if out_v is not None else None, out_v.shape[2] if out_v is not None else 0,
                                  out_i.ctypes.data if out_i is not None else None, out_i.shape[2] if out_i is not None else 0,
                                  r.ctypes.data if len(r) else None, len(r), pt.ctypes.data if len(pt) else None, len(pt) if n_pts is None else n_pts,
                                  timing.ctypes.data if timing is not None else None,
                                  (timing.shape[1] if timing is not None else 0) if n_timing is None else n_timing, rows.ctypes.data, stride, int(have_out),
                                  work_bytes, threads or L.spicey_values_host_threads(), grid, err, 256)
    if rc != abi.OK:
        assert rc == abi.ERR_BAD_DESC and (rows == SENTINEL).all()
        raise Refused(err.value.decode())
    return rows[:, :len(r)]


def waveforms(n_inst, n_points, n_v, n_i, seed):
    """Seeded samples, most of them from nine values a quarter apart — equal samples (first-occurrence ties) occur all the
    time — the rest continuous.  Column 0 of both arrays is a sinusoid of three periods per run with a phase of its
    instance's own (what the find requests' edges cross)."""
    rng = np.random.default_rng(seed)

    def one(n, shift):
        q = rng.integers(-4, 5, size=(n_inst, n_points, n)) / 4.0
        c = rng.uniform(-0.99, 0.99, size=(n_inst, n_points, n))
        a = np.where(rng.random((n_inst, n_points, n)) < 0.7, q, c)
        s = np.arange(n_points)[None, :] / max(n_points - 1, 1)
        a[:, :, 0] = np.sin(2.0 * np.pi * 3.0 * s + 0.7 * np.arange(n_inst)[:, None] + shift)
        return np.ascontiguousarray(a)
    return one(n_v, 0.0), one(n_i, 1.1)


# the edges the find requests look up: (x_signal, x_col, x_col_ref, dir, n, level); the fourth is above every sample
EDGES = [(0, 0, -1, 1, 1, 0.3), (0, 0, -1, -1, 1, -0.5), (1, 0, -1, 0, 2, 0.85), (0, 0, -1, 1, 1, 1.5), (1, 0, -1, 1, -1, 0.0), (1, 0, 1, 1, 1, 0.1)]


def timing_list():
    """One targ-only request over the whole run per edge of EDGES."""
    return make_timing_reqs([(0, -1, None, (sig, col, ref, d, n, abi.TIMING_ABS, 0, 0, level), False) for sig, col, ref, d, n, level in EDGES])


def timing_rows(out_v, out_i, dt):
    """The rows the timing pass gives for timing_list(), by its numpy definition: [n_inst][len(EDGES)][8]."""
    return reduce_reference_timing(out_v, out_i, timing_list(), dt)


def point_table(n_points, count, seed):
    """`count` points: the run's first and last interval, f = 0 and f = 1 among them, the rest anywhere."""
    rng = np.random.default_rng(seed)
    k = rng.integers(0, n_points - 1, size=count)
    f = rng.random(count)
    k[:4] = (0, 0, n_points - 2, n_points - 2)
    f[:4] = (0.0, 1.0, 0.0, 1.0)
    f[4:8] = (0.5, 2.0 ** -53, 1.0 - 2.0 ** -53, 0.25)
    return make_value_points(list(zip(k.tolist(), f.tolist())))


def request_pool(n_points, n_v, n_i, count, seed, n_pts):
    """`count` requests, request k of kind k % 3, from out_i for odd k // 3, with a reference column for odd k // 6 (different
    from the column where the array has two, else the column itself: a signal of exact zeros).  Traces: windows in turn
    the whole run, random sub-windows (they start anywhere in a chunk) and windows of c - 1, c, c + 1 and 2c - 2 .. 2c + 2
    samples from a random start, so that with B = 1 and B = 2 a bucket ends one before, on and one after its first
    sub-chunk's end; B in turn 1, 2, 3, 7, 64, 65, n, clipped to n.  Points: a random run of the table.  Finds: the edges
    of EDGES in turn.  From request 60 on every fifth request repeats an earlier one."""
    rng = np.random.default_rng(seed)
    c = chunk()
    rows = []
    lengths = [c - 1, c, c + 1, 2 * c - 2, 2 * c - 1, 2 * c, 2 * c + 1, 2 * c + 2]
    for k in range(count):
        if k >= 60 and k % 5 == 4:
            rows.append(rows[int(rng.integers(0, k))])
            continue
        kind, sig, ref = k % 3, (k // 3) % 2, bool((k // 6) % 2)
        n = n_i if sig else n_v
        col = int(rng.integers(0, n))
        cr = -1 if not ref else (col + 1 + int(rng.integers(0, n - 1))) % n if n > 1 else col
        if kind == abi.VAL_TRACE:
            j = k // 3
            w = j % 3
            if w == 0:
                s0, s1 = 0, n_points - 1
            elif w == 1:
                s0 = int(rng.integers(0, n_points))
                s1 = int(rng.integers(s0, n_points))
            else:
                ln = min(lengths[(j // 3) % len(lengths)], n_points)
                s0 = int(rng.integers(0, n_points - ln + 1))
                s1 = s0 + ln - 1
            ns = s1 - s0 + 1
            # (the windows of planted lengths: one bucket of c - 1, c, c + 1 steps, or two that split 2c - 2 .. 2c + 2)
            B = min((1 if (j // 3) % len(lengths) < 3 else 2) if w == 2 else [1, 2, 3, 7, 64, 65, ns][(j // 3) % 7], ns)
            rows.append((kind, sig, col, cr, 0, 0, -1, 0, s0, -1 if w == 0 and k % 2 else s1, 0, 0, B))
        elif kind == abi.VAL_POINTS:
            first = int(rng.integers(0, n_pts))
            rows.append((kind, sig, col, cr, 0, 0, -1, 0, 0, 0, first, int(rng.integers(1, n_pts - first + 1)), 0))
        else:
            t = (k // 3) % len(EDGES)
            rows.append((kind, sig, col, cr) + EDGES[t][:3] + (t, 0, 0, 0, 0, 0))
    return make_value_reqs(rows)


def bits_equal(a, b):
    a = np.ascontiguousarray(a, dtype=np.float64)
    b = np.ascontiguousarray(b, dtype=np.float64)
    return (a.view(np.int64) == b.view(np.int64)) | (np.isnan(a) & np.isnan(b))


def check_against_reference(got, out_v, out_i, reqs, pts, dt, timing):
    """Every double of every row, the zeros behind a request's own included, bit for bit against reduce_reference_values."""
    ref = reduce_reference_values(out_v, out_i, reqs, pts, dt, timing)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    same = bits_equal(got, ref)
    assert same.all(), (np.argwhere(~same)[:5], [reqs[r] for r in sorted({int(a[1]) for a in np.argwhere(~same)[:5]})])
    return ref
