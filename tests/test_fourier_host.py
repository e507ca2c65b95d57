"""The harmonics pass on the CPU: spicey_amd/csrc/fourier_exec.h — the code the kernels of fourier.hip run — through the
harness of tests/fourier_host (an emulation of the kernels' lane, tile and chunk mapping) against reduce_reference_fourier,
the numpy definition.  The bound is pyfourier.check_against_reference's: C0 within n 2^-52 sum |x|, every C_h and S_h
within (n + 8) 2^-52 sum |x| (any summation order on both sides, one rounding per product, 4 ulp per twiddle for a libm
that is not numpy's); its derivation is in that docstring."""
import math
import os
import sys

import numpy as np
import pytest

from conftest import REPO, bits_equal
from spicey_amd.measure import make_four_reqs

for _d in ("measure_host", "fourier_host"):
    sys.path.insert(0, os.path.join(REPO, "tests", _d))
import pyfourier as pf  # noqa: E402
import pymeasure as pm  # noqa: E402

N_INST, N_I, DT = 3, 5, 1e-6


def n_points_list():
    c = pf.chunk()
    return [2, c - 1, c, c + 1, 3 * c + 7]


def _basis_of(q, n_points):
    return (float(q["f0"]), int(q["step_from"]), n_points - 1 if int(q["step_to"]) == -1 else int(q["step_to"]))


@pytest.mark.parametrize("n_v", [1, 2, 63, 64, 65, 130])
def test_harness_equals_reference_and_a_row_stands_alone(n_v):
    assert pf.chunk() == pm.chunk()  # (one chunking for every reduction)
    worst_tw = 0.0
    for n_points in n_points_list():
        out_v, out_i = pm.waveforms(N_INST, n_points, n_v, N_I, seed=1000 * n_v + n_points)  # (the nine quarter-spaced values)
        pool = pf.request_pool(n_points, n_v, N_I, 300, DT, seed=n_v + n_points)
        bases = {_basis_of(q, n_points) for q in pool}
        assert len(bases) >= 3 and (n_points == 2 or len({b - a for _, a, b in bases}) >= 3)
        assert {int(q["signal"]) for q in pool} == {0, 1} and {int(q["n_harm"]) for q in pool} == {1, 9, 16}
        assert any(int(q["col_ref"]) >= 0 for q in pool) and len({q.tobytes() for q in pool}) < len(pool)
        full = pf.run(out_v, out_i, pool, DT)
        worst_tw = max(worst_tw, pf.check_against_reference(full, out_v, out_i, pool, DT))
        w = full.shape[2]
        for count in (1, 65):  # (shorter lists of the same pool; rows are padded to the list's own widest request)
            part = pf.run(out_v, out_i, pool[:count], DT)
            pf.check_against_reference(part, out_v, out_i, pool[:count], DT)
            assert bits_equal(part, full[:, :count, :part.shape[2]]).all(), (n_points, count)
        # a request's row does not depend on the rest of the list: alone, and 65 of them in another order
        for k in (0, 1, 7, 150):
            alone = pf.run(out_v, out_i, pool[k:k + 1], DT)
            assert bits_equal(alone, full[:, k:k + 1, :alone.shape[2]]).all(), (n_points, k)
        perm = np.random.default_rng(n_v).permutation(300)[:65]
        sub = pf.run(out_v, out_i, pool[perm], DT)
        assert bits_equal(sub, full[:, perm, :sub.shape[2]]).all(), n_points
        # nor on the other members of its basis: the same request next to one with more harmonics, and with fewer
        q = pool[0].copy()
        q["n_harm"] = 9
        lone = pf.run(out_v, out_i, [q], DT)
        for other in (16, 3):
            q2 = q.copy()
            q2["n_harm"], q2["col"] = other, (int(q["col"]) + 1) % n_v
            pair = pf.run(out_v, out_i, np.array([q2, q, q2]), DT)
            assert bits_equal(pair[:, 1, :19], lone[:, 0]).all() and (pair[:, 1, 19:] == 0).all(), (n_points, other)
        # nor on the emulated launch: workgroup size and grid
        for threads, grid in ((64, 0), (1024, 0), (1, 0), (256, 1), (128, 3), (32, 5)):
            assert bits_equal(pf.run(out_v, out_i, pool[:65], DT, threads=threads, grid=grid, out_stride=w), full[:, :65]).all(), (n_points, threads, grid)
        # nor on n_inst: an instance's samples alone, and among others
        assert bits_equal(pf.run(out_v[1:2], out_i[1:2], pool[:65], DT, out_stride=w), full[1:2, :65]).all(), n_points
        more_v, more_i = np.concatenate([out_v[::-1], out_v, out_v[:1]]), np.concatenate([out_i[::-1], out_i, out_i[:1]])
        got = pf.run(more_v, more_i, pool[:65], DT, out_stride=w)
        assert bits_equal(got[3:6], full[:, :65]).all() and bits_equal(got[6], full[0, :65]).all() and bits_equal(got[2], full[0, :65]).all(), n_points
    print(f"largest twiddle distance, this libm against numpy: {worst_tw} ulp of 1")
    assert worst_tw <= 4.0  # (what the bound allows for)


def test_the_combining_order_is_the_documented_one():
    """The definition written out again in Python — chunks of C steps from the window's first, sums from 0.0 in step order,
    partials added in ascending chunk order starting from chunk 0's, the library's own twiddles — gives the harness's
    bits; a wider row is zero-filled; the absolute step, not the window's, enters the twiddle."""
    c = pf.chunk()
    n_points = 3 * c + 7
    out_v, out_i = pm.waveforms(1, n_points, 3, 2, seed=11)
    f0 = 1.0 / (40.0 * DT)
    s0, s1, H = 37, 2 * c + 100, 3
    got = pf.run(out_v, out_i, make_four_reqs([(0, 2, 0, H, s0, s1, f0)]), DT, out_stride=12)[0, 0]
    x = (out_v[0, :, 2] - out_v[0, :, 0]).tolist()
    f0dt = f0 * DT
    want = []
    for j in range(1 + 2 * H):
        parts = []
        for lo in range(s0, s1, c):
            acc = 0.0
            for s in range(lo, min(lo + c, s1)):
                t = 1.0 if j == 0 else pf.twiddle((j + 1) // 2, s, f0dt)[(j + 1) % 2]
                acc = acc + (x[s] if j == 0 else x[s] * t)
            parts.append(acc)
        tot = parts[0]
        for p in parts[1:]:
            tot = tot + p
        want.append(tot)
    assert len(want) == 7 and bits_equal(got[:7], want).all() and (got[7:].view(np.int64) == 0).all()
    # the twiddle itself: the three operations of the header, then the host's libm
    for h, s in ((1, 0), (3, 41), (16, 10 ** 9 + 7)):
        r = float(h * s) * f0dt
        r = r - math.floor(r)
        cs = pf.twiddle(h, s, f0dt)
        assert abs(cs[0] - math.cos(2.0 * math.pi * r)) <= 4 * pf.U and abs(cs[1] - math.sin(2.0 * math.pi * r)) <= 4 * pf.U
    # a pure cosine at the second harmonic, over whole periods that do not start at step 0: C2 = N / 2, the rest ~ 0
    k = np.arange(n_points)
    y = np.cos(2 * np.pi * 2 * f0 * k * DT + 0.3)[None, :, None]
    row = pf.run(y, None, make_four_reqs([(0, 0, -1, 3, 17, 17 + 400, f0)]), DT)[0, 0]
    a2, b2 = 2 * row[3] / 400, 2 * row[4] / 400
    assert abs(math.hypot(a2, b2) - 1.0) < 1e-12 and abs(math.atan2(-b2, a2) - 0.3) < 1e-12
    assert max(abs(row[0]), abs(row[1]), abs(row[2]), abs(row[5]), abs(row[6])) < 1e-10


def test_refused_request_lists():
    out_v, out_i = pm.waveforms(2, 10, 3, 2, seed=1)
    f0 = 1.0 / (40.0 * DT)
    ok = (0, 0, -1, 2, 0, -1, f0)
    pf.run(out_v, out_i, make_four_reqs([ok]), DT)
    bad = [(2, 0, -1, 2, 0, -1, f0), (-1, 0, -1, 2, 0, -1, f0),  # signal
           (0, 3, -1, 2, 0, -1, f0), (0, -1, -1, 2, 0, -1, f0), (0, 0, 3, 2, 0, -1, f0), (0, 0, -2, 2, 0, -1, f0), (1, 2, -1, 2, 0, -1, f0),  # columns
           (0, 0, -1, 2, -1, 5, f0), (0, 0, -1, 2, 0, 10, f0), (0, 0, -1, 2, 5, 5, f0), (0, 0, -1, 2, 6, 5, f0), (0, 0, -1, 2, 9, -1, f0),
           (0, 0, -1, 2, 0, -2, f0),  # windows
           (0, 0, -1, 0, 0, -1, f0), (0, 0, -1, 17, 0, -1, f0), (0, 0, -1, -3, 0, -1, f0),  # n_harm
           (0, 0, -1, 2, 0, -1, 0.0), (0, 0, -1, 2, 0, -1, -f0), (0, 0, -1, 2, 0, -1, float("inf")), (0, 0, -1, 2, 0, -1, float("nan")),  # f0
           (0, 0, -1, 2, 0, -1, 0.26 / DT), (0, 0, -1, 16, 0, -1, 1.01 / (32 * DT))]  # above Nyquist
    for b in bad:
        with pytest.raises(pf.Refused, match="fourier"):
            pf.run(out_v, out_i, make_four_reqs([ok, b]), DT, out_stride=33, fill=7.0)
    pf.run(out_v, out_i, make_four_reqs([(0, 0, -1, 2, 0, -1, 0.2499 / DT), (0, 0, -1, 16, 0, -1, 0.999 / (32 * DT))]), DT)  # just under Nyquist: accepted
    with pytest.raises(pf.Refused, match="fourier"):
        pf.run(out_v, None, make_four_reqs([(1, 0, -1, 2, 0, -1, f0)]), DT)  # a current without a current buffer
    with pytest.raises(pf.Refused, match="fourier"):
        pf.run(out_v, out_i, make_four_reqs([]), DT)  # n_req = 0
    for stride in (4, 0, -1):
        with pytest.raises(pf.Refused, match="fourier"):
            pf.run(out_v, out_i, make_four_reqs([ok]), DT, out_stride=stride)  # a row shorter than 1 + 2 n_harm
    for dt in (0.0, -DT, float("nan"), float("inf")):
        with pytest.raises(pf.Refused, match="fourier"):
            pf.run(out_v, out_i, make_four_reqs([ok]), dt)
    need = pf.workspace_bytes(2, 10, make_four_reqs([ok]))
    # table 256 | bases 256 | twiddles 9 steps x 2 harmonics x 16 B = 288 -> 512 | partials 2 inst x 1 chunk x 5 x 1 req x 8 B
    assert need == 256 + 256 + 512 + 2 * 5 * 8
    pf.run(out_v, out_i, make_four_reqs([ok]), DT, work_bytes=need)
    with pytest.raises(pf.Refused, match="fourier"):
        pf.run(out_v, out_i, make_four_reqs([ok]), DT, work_bytes=need - 8)  # a short workspace
    assert pf.workspace_bytes(0, 10, make_four_reqs([ok])) == -1 and pf.workspace_bytes(2, 10, make_four_reqs([])) == -1
    assert pf.workspace_bytes(2, 10, make_four_reqs([bad[8]])) == -1 and pf.workspace_bytes(2, 10, make_four_reqs([bad[14]])) == -1
    L = pf.lib()  # null buffers
    r = make_four_reqs([ok])
    err = pf.C.create_string_buffer(256)
    out = np.zeros((2, 1, 5))
    assert L.spicey_four_host_run(2, 10, DT, None, 3, None, 0, r.ctypes.data, 1, out.ctypes.data, 5, -1, 256, 0, err, 256) == 2 and b"fourier" in err.value
    assert L.spicey_four_host_run(2, 10, DT, out_v.ctypes.data, 3, None, 0, r.ctypes.data, 1, None, 5, -1, 256, 0, err, 256) == 2 and b"fourier" in err.value
