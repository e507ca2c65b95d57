"""ctypes view of the CPU harness of the AC measurements (tests/ac_measure_host/harness.cpp) and the buffers and request
lists the host and GPU tests share."""
import ctypes as C
import os

import numpy as np

import harness_build
from spicey_amd import abi
from spicey_amd.ac_measure import make_ac_reqs

HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None

N_INST, N_I = 3, 4
N_VS = (1, 2, 5)
N_FREQS = (1, 2, 63, 64, 65, 129, 300)  # the lane-count edges


def lib():
    global _LIB
    if _LIB is None:
        L = harness_build.load(HERE, "libspicey_ac_measure_host.so")
        L.spicey_acm_host_lanes.restype = C.c_int32
        L.spicey_acm_host_workspace_bytes.restype = C.c_int64
        L.spicey_acm_host_workspace_bytes.argtypes = [C.c_int32, C.c_int64, C.c_int32]
        L.spicey_acm_host_run.restype = C.c_int32
        L.spicey_acm_host_run.argtypes = [C.c_int32, C.c_int64, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p,
                                          C.c_int32, C.c_int64, C.c_char_p, C.c_int32]
        _LIB = L
    return _LIB


class Refused(ValueError):
    pass


def run(out_v, out_i, reqs, lanes=None, waves=0):
    """meas [n_inst][n_req][8] of the harness; lanes / waves: the emulated launch (default: the kernel's own lane count, one
    wave per pair)."""
    L = lib()
    out_v = np.ascontiguousarray(out_v, dtype=np.complex128)
    out_i = np.ascontiguousarray(out_i, dtype=np.complex128) if out_i is not None else None
    r = np.ascontiguousarray(reqs, dtype=abi.AC_MEAS_REQ_DTYPE).reshape(-1)
    ni, nf, n_v = out_v.shape
    meas = np.full((ni, max(len(r), 1), 8), np.nan)
    err = C.create_string_buffer(256)
    rc = L.spicey_acm_host_run(ni, nf, out_v.ctypes.data, n_v, out_i.ctypes.data if out_i is not None else None,
                               out_i.shape[2] if out_i is not None else 0, r.ctypes.data if len(r) else None, len(r), meas.ctypes.data,
                               lanes or L.spicey_acm_host_lanes(), waves, err, 256)
    if rc == -1:
        raise AssertionError("the lanes of a wave disagree after the butterfly")
    if rc != abi.OK:
        raise Refused(err.value.decode())
    return meas[:, :len(r)]


def buffers(n_freq, n_v, seed, n_inst=N_INST, n_i=N_I):
    """Seeded complex samples, most parts from nine values a quarter apart — equal extremes over whole plateaus (the first
    occurrence must win) and samples exactly on a level occur all the time — the rest continuous.  Planted on top: a NaN
    sample in the middle of every column of out_v's instance 1 and as the FIRST sample of out_i's column 1 of instance 2,
    and one exactly zero sample (a zero denominator) in out_v's last column of instance 0."""
    rng = np.random.default_rng(seed)

    def one(n):
        def part():
            q = rng.integers(-4, 5, size=(n_inst, n_freq, n)) / 4.0
            c = rng.uniform(-0.99, 0.99, size=(n_inst, n_freq, n))
            return np.where(rng.random((n_inst, n_freq, n)) < 0.7, q, c)
        return np.ascontiguousarray(part() + 1j * part())
    v, i = one(n_v), one(n_i)
    if n_freq >= 3:
        v[1, n_freq // 2, :] = complex(np.nan, 0.25)
        v[0, n_freq // 3, n_v - 1] = 0.0
        a, b = n_freq // 4, min(n_freq // 4 + 9, n_freq)
        v[2, a:b, 0] = 1.25 + 1.25j      # a plateau at the largest |H|^2 and re the pool can see on column 0
        i[0, a:b, 2] = -1.25 - 1.25j     # and one at the smallest re / im
    i[2, 0, 1] = complex(np.nan, np.nan)
    return v, i


def windows(n_freq):
    """(from, to) pairs: the whole sweep (to = -1 and explicit), single points, windows that start and end on and next to a
    multiple of the lane count."""
    marks = sorted({k for k in (0, 1, 7, 62, 63, 64, 65, 127, 128, 129, n_freq // 2, n_freq - 2, n_freq - 1) if 0 <= k < n_freq})
    out = [(0, -1), (0, n_freq - 1)]
    out += [(k, k) for k in marks]
    out += [(a, b) for a in marks for b in marks if a < b]
    return out


LEVELS = (0.25, 0.5, 1.0, -0.5, 0.0, 0.0625, 2.0)


def request_pool(n_freq, n_v, n_i, count=200, seed=0):
    """`count` requests cycling through the windows, both kinds, every `what`, `dir`, `which` and `rel`, voltage and current
    signals, difference signals and quotients (also of a voltage by a current); every seventh one repeats an earlier one."""
    rng = np.random.default_rng(seed)
    wins = windows(n_freq)
    rows = []
    for k in range(count):
        if k % 7 == 6:
            rows.append(rows[int(rng.integers(0, len(rows)))])
            continue
        a, b = wins[k % len(wins)]
        sig = (k // 5) % 2
        n = n_i if sig else n_v
        col = (k * 3 + k // 4) % n
        col_ref = int(rng.integers(0, n)) if k % 3 == 2 else -1
        if k % 4 == 1:
            dsig = (k // 8) % 2
            dn = n_i if dsig else n_v
            den = (dsig, (k // 2) % dn, int(rng.integers(0, dn)) if k % 8 == 5 else -1)
        elif k % 16 == 2:
            den = (0, n_v - 1, -1)  # (the column with the zero sample)
        else:
            den = (-1, 0, 0)
        what = (k // 2) % 3
        if k % 2 == 0:
            rows.append((sig, col, col_ref) + den + (what, abi.AC_MEAS_EXTREMA, a, b, 0.0, 0, 0, 0))
        else:
            rel = (k // 6) % 2
            rows.append((sig, col, col_ref) + den + (what, abi.AC_MEAS_CROSS, a, b, LEVELS[(k // 2) % len(LEVELS)], (1, -1, 0)[(k // 2) % 3],
                                                     (k // 4) % 2, rel))
    return make_ac_reqs(rows)


def refusals(n_freq, n_v, n_i):
    """(name, rows, have_i) of request lists no launch accepts; the good request they are made from is accepted."""
    good = (0, 0, -1, -1, 0, 0, 0, abi.AC_MEAS_CROSS, 0, -1, 0.5, 1, 0, 0)

    def mod(**kw):
        names = ("num_signal", "num_col", "num_col_ref", "den_signal", "den_col", "den_col_ref", "what", "kind", "k_from", "k_to", "level", "dir",
                 "which", "rel")
        r = list(good)
        for k, v in kw.items():
            r[names.index(k)] = v
        return tuple(r)
    cases = [("kind", mod(kind=2)), ("num_signal", mod(num_signal=2)), ("den_signal", mod(den_signal=-2)), ("what", mod(what=3)), ("dir", mod(dir=2)),
             ("which", mod(which=2)), ("rel", mod(rel=-1)), ("num_col", mod(num_col=n_v)), ("num_col_ref", mod(num_col_ref=n_v)),
             ("den_col", mod(den_signal=0, den_col=-1)), ("den_col_ref", mod(den_signal=1, den_col=0, den_col_ref=n_i)),
             ("window_past", mod(k_to=n_freq)), ("window_neg", mod(k_from=-1)), ("window_order", mod(k_from=1, k_to=0))]
    out = [(name, make_ac_reqs([good, row]), True) for name, row in cases]
    out.append(("no_current_buffer", make_ac_reqs([mod(num_signal=1)]), False))
    out.append(("den_no_current_buffer", make_ac_reqs([mod(den_signal=1)]), False))
    res = make_ac_reqs([good])
    res["reserved"] = 1
    out.append(("reserved", res, True))
    out.append(("empty", make_ac_reqs([]), True))
    return make_ac_reqs([good]), out
