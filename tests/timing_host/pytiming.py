"""ctypes view of the CPU harness of the edge-timing pass (tests/timing_host/harness.cpp), the request pool the host and GPU
tests share, and the sanitized self-test's build."""
import ctypes as C
import os
import sys

import numpy as np

import harness_build
from spicey_amd import abi
from spicey_amd.measure import make_timing_reqs

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "measure_host"))
import pymeasure as pm  # noqa: E402

_LIB = None


def lib():
    global _LIB
    if _LIB is None:
        L = harness_build.load(HERE, "libspicey_timing_host.so")
        L.spicey_tim_host_chunk.restype = C.c_int32
        L.spicey_tim_host_threads.restype = C.c_int32
        L.spicey_tim_host_workspace_bytes.restype = C.c_int64
        L.spicey_tim_host_workspace_bytes.argtypes = [C.c_int32, C.c_int64, C.c_void_p, C.c_int32]
        L.spicey_tim_host_run.restype = C.c_int32
        L.spicey_tim_host_run.argtypes = [C.c_int32, C.c_int64, C.c_double, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32,
                                          C.c_void_p, C.c_int64, C.c_int32, C.c_int64, C.c_char_p, C.c_int32]
        _LIB = L
    return _LIB


def selftest_path() -> str:
    """The sanitized stand-alone program (selftest.cpp + harness.cpp), built on first use."""
    harness_build.make(HERE, "_build/selftest")
    return os.path.join(HERE, "_build", "selftest")


def chunk() -> int:
    return lib().spicey_tim_host_chunk()


class Refused(ValueError):
    pass


def _r(reqs):
    return np.ascontiguousarray(reqs, dtype=abi.TIMING_REQ_DTYPE).reshape(-1)


def workspace_bytes(n_inst, n_points, reqs) -> int:
    r = _r(reqs)
    return lib().spicey_tim_host_workspace_bytes(n_inst, n_points, r.ctypes.data if len(r) else None, len(r))


def run(out_v, out_i, reqs, dt, threads=None, grid=0, work_bytes=-1, fill=np.nan):
    """Rows [n_inst][n_req][8] of the harness; threads / grid: the emulated launch (default: the kernels' own).  A refusal
    raises Refused with the result buffer still holding `fill`."""
    L = lib()
    out_v = np.ascontiguousarray(out_v, dtype=np.float64)
    out_i = np.ascontiguousarray(out_i, dtype=np.float64) if out_i is not None else None
    r = _r(reqs)
    ni, n_points, n_v = out_v.shape
    out = np.full((ni, max(len(r), 1), 8), fill)
    err = C.create_string_buffer(256)
    rc = L.spicey_tim_host_run(ni, n_points, dt, out_v.ctypes.data, n_v, out_i.ctypes.data if out_i is not None else None,
                               out_i.shape[2] if out_i is not None else 0, r.ctypes.data if len(r) else None, len(r), out.ctypes.data, work_bytes,
                               threads or L.spicey_tim_host_threads(), grid, err, 256)
    if rc != abi.OK:
        assert rc == abi.ERR_BAD_DESC and pm.bits_equal(out, np.full_like(out, fill)).all()
        raise Refused(err.value.decode())
    return out[:, :len(r)]


def windows(n_points):
    """(from, to) pairs with at least one interval: the whole run (to = -1 and explicit), windows that start and end in the
    middle of a chunk and on chunk edges, and windows of two points there."""
    out = [(a, b) for a, b in pm.windows(n_points) if b == -1 or a < b]
    c = chunk()
    return out + [(s, s + 1) for s in sorted({0, c - 1, c, n_points - 2}) if 0 <= s < n_points - 1]


ABS_LEVELS = (0.25, 0.1, -0.5, 0.0)
REL_FRACS = (0.25, 0.5, 0.75, 0.25, 0.5, 0.75, 0.5, 0.0, 1.0, 1.25)  # quarters, and one beyond the swing
NS = (1, 1, 1, 1, -1, -1, 2, 2, -2, 3, -3, 4)   # -3 .. 4: most windows hold that many crossings, the short ones do not


def request_pool(n_points, n_v, n_i, count, seed):
    """`count` requests cycling through the windows, with and without a trig and both targ_from_trig values; each edge draws
    its signal, column, reference column, direction, occurrence, level kind, level and base window (the whole run, one
    point, a sub-window); every seventh request repeats an earlier one."""
    rng = np.random.default_rng(seed)
    wins = windows(n_points)
    subs = [(a, b) for a, b in pm.windows(n_points) if b != -1]

    def one_edge():
        sig = int(rng.integers(0, 2))
        n = n_i if sig else n_v
        col = int(rng.integers(0, n))
        col_ref = int(rng.integers(0, n)) if rng.integers(0, 3) == 2 else -1
        kind = int(rng.integers(0, 3))
        level = ABS_LEVELS[int(rng.integers(0, 4))] if kind == 0 else REL_FRACS[int(rng.integers(0, len(REL_FRACS)))]
        b0, b1 = (0, 0) if kind == 0 else ((0, -1), (0, n_points - 1), subs[int(rng.integers(0, len(subs)))])[int(rng.integers(0, 3))]
        return (sig, col, col_ref, (1, -1, 0)[int(rng.integers(0, 3))], NS[int(rng.integers(0, len(NS)))], kind, b0, b1, level)

    rows = []
    for k in range(count):
        if k % 7 == 6:
            rows.append(rows[int(rng.integers(0, len(rows)))])
            continue
        a, b = (0, -1) if k % 4 == 0 else wins[k % len(wins)]  # (a quarter of the requests over the whole run)
        rows.append((a, b, one_edge() if k % 2 else None, one_edge(), (k // 2) % 2 if k % 2 else 0))
    return make_timing_reqs(rows)


def found_every_edge(ref, reqs):
    """[n_inst][n_req] bool: the row found every edge its request asks for."""
    has_trig = _r(reqs)["has_trig"].astype(bool)[None, :]
    return (ref[:, :, 3] >= 0) & ((ref[:, :, 0] >= 0) | ~has_trig)
