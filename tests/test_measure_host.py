"""The waveform measurements on the CPU: spicey_amd/csrc/measure_exec.h — the code the kernels of measure.hip run —
through the harness of tests/measure_host (an emulation of the kernels' lane and chunk mapping) against reduce_reference,
the numpy definition.  Order-free fields bit for bit; the two sums within the bound that holds for any summation order:
|err| <= n 2^-52 sum |x| and (n + 1) 2^-52 sum x^2 (n terms: n - 1 additions of relative error 2^-53 each compound to less
than n 2^-53, the squares add one rounding; a factor 2 is left for the reference's own sum)."""
import os
import sys

import numpy as np
import pytest

from conftest import REPO, bits_equal
from spicey_amd.measure import make_reqs

sys.path.insert(0, os.path.join(REPO, "tests", "measure_host"))
import pymeasure as pm  # noqa: E402

N_INST, N_I, DT = 3, 5, 1e-6


def n_points_list():
    c = pm.chunk()
    return [1, 2, c - 1, c, c + 1, 3 * c + 7]


@pytest.mark.parametrize("n_v", [1, 2, 63, 64, 65, 130])
def test_harness_equals_reference_and_a_request_stands_alone(n_v):
    for n_points in n_points_list():
        out_v, out_i = pm.waveforms(N_INST, n_points, n_v, N_I, seed=1000 * n_v + n_points)
        pool = pm.request_pool(n_points, n_v, N_I, 300, seed=n_v + n_points)
        kinds = {(int(q["kind"]), int(q["signal"]), int(q["col_ref"]) >= 0) for q in pool}
        assert len(kinds) == 8 and {int(q["dir"]) for q in pool if q["kind"] == 1} == {1, -1, 0}
        assert len({q.tobytes() for q in pool}) < len(pool)  # (the same request more than once)
        full = pm.run(out_v, out_i, pool, DT)
        pm.check_against_reference(full, out_v, out_i, pool, DT)
        # a request's 8 doubles do not depend on the rest of the list: alone, and 65 of them in another order
        for k in (0, 1, 7, 150):
            assert bits_equal(pm.run(out_v, out_i, pool[k:k + 1], DT), full[:, k:k + 1]).all(), (n_points, k)
        perm = np.random.default_rng(n_v).permutation(300)[:65]
        assert bits_equal(pm.run(out_v, out_i, pool[perm], DT), full[:, perm]).all(), n_points
        # nor on the emulated launch: workgroup size and grid
        for threads, grid in ((64, 0), (1024, 0), (1, 0), (256, 1), (128, 3)):
            assert bits_equal(pm.run(out_v, out_i, pool[:65], DT, threads=threads, grid=grid), full[:, :65]).all(), (n_points, threads, grid)
        # nor on n_inst: an instance's samples alone, and among others
        assert bits_equal(pm.run(out_v[1:2], out_i[1:2], pool[:65], DT), full[1:2, :65]).all(), n_points
        more_v, more_i = np.concatenate([out_v[::-1], out_v, out_v[:1]]), np.concatenate([out_i[::-1], out_i, out_i[:1]])
        got = pm.run(more_v, more_i, pool[:65], DT)
        assert bits_equal(got[3:6], full[:, :65]).all() and bits_equal(got[6], full[0, :65]).all() and bits_equal(got[2], full[0, :65]).all(), n_points


def test_ties_and_samples_on_the_level_occur_and_are_decided_by_the_rule():
    c = pm.chunk()
    n_points = 3 * c + 7
    out_v, out_i = pm.waveforms(N_INST, n_points, 2, N_I, seed=5)
    x = out_v[0, :, 0]
    assert np.count_nonzero(x == x.min()) > 1 or np.count_nonzero(x == x.max()) > 1
    assert np.count_nonzero(x == 0.25) > 0
    # the extreme planted again in a later chunk: the first occurrence is reported
    out_v[0, 5, 0] = out_v[0, 2 * c + 3, 0] = 9.0
    out_v[0, c - 1, 0] = out_v[0, c, 0] = -9.0  # (either side of a chunk edge)
    m = pm.run(out_v, out_i, make_reqs([(0, 0, 0, -1, 0, -1, 0.0, 0)]), DT)[0, 0]
    assert (m[0], m[1], m[2], m[3]) == (-9.0, 9.0, float(c - 1), 5.0)
    # a crossing whose interval straddles two chunks is counted once, in exactly one of them
    y = np.zeros((1, n_points, 1))
    y[0, c:, 0] = 1.0  # the only rise: steps c - 1 -> c
    m = pm.run(y, None, make_reqs([(1, 0, 0, -1, 0, -1, 0.5, 1), (1, 0, 0, -1, c - 1, c, 0.5, 0), (1, 0, 0, -1, c, -1, 0.5, 0),
                                   (1, 0, 0, -1, 0, c - 1, 0.5, 0)]), DT)[0]
    t = ((c - 1) + 0.5) * DT
    assert list(m[0][:3]) == [1.0, t, t] and list(m[1][:3]) == [1.0, t, t]
    assert list(m[2][:3]) == [0.0, -1.0, -1.0] and list(m[3][:3]) == [0.0, -1.0, -1.0]
    # x == level exactly: x_k < level <= x_k+1 is a rise that lands ON step k + 1; leaving the level upwards is none
    z = np.array([0.0, 0.5, 0.5, 1.0, 0.5, 0.0])[None, :, None]
    m = pm.run(z, None, make_reqs([(1, 0, 0, -1, 0, -1, 0.5, 1), (1, 0, 0, -1, 0, -1, 0.5, -1), (1, 0, 0, -1, 0, -1, 0.5, 0)]), DT)[0]
    assert list(m[0][:3]) == [1.0, 1.0 * DT, 1.0 * DT]
    assert list(m[1][:3]) == [1.0, 4.0 * DT, 4.0 * DT]
    assert list(m[2][:3]) == [2.0, 1.0 * DT, 4.0 * DT]


def test_refused_request_lists():
    out_v, out_i = pm.waveforms(2, 10, 3, 2, seed=1)
    ok = (0, 0, 0, -1, 0, -1, 0.0, 0)
    pm.run(out_v, out_i, make_reqs([ok]), DT)
    bad = [(2, 0, 0, -1, 0, -1, 0.0, 0), (0, 2, 0, -1, 0, -1, 0.0, 0), (1, 0, 0, -1, 0, -1, 0.0, 2),  # kind, signal, dir
           (0, 0, 3, -1, 0, -1, 0.0, 0), (0, 0, -1, -1, 0, -1, 0.0, 0), (0, 0, 0, 3, 0, -1, 0.0, 0), (0, 1, 2, -1, 0, -1, 0.0, 0),  # columns
           (0, 0, 0, -1, -1, 5, 0.0, 0), (0, 0, 0, -1, 0, 10, 0.0, 0), (0, 0, 0, -1, 6, 5, 0.0, 0), (0, 0, 0, -1, 0, -2, 0.0, 0)]  # windows
    for b in bad:
        with pytest.raises(pm.Refused):
            pm.run(out_v, out_i, make_reqs([ok, b]), DT)
    with pytest.raises(pm.Refused):
        pm.run(out_v, None, make_reqs([(0, 1, 0, -1, 0, -1, 0.0, 0)]), DT)  # a current without a current buffer
    with pytest.raises(pm.Refused):
        pm.run(out_v, out_i, make_reqs([]), DT)  # n_req = 0
    L = pm.lib()
    assert L.spicey_meas_host_workspace_bytes(0, 10, 1) == -1 and L.spicey_meas_host_workspace_bytes(1, 10, 0) == -1
    c = pm.chunk()
    assert L.spicey_meas_host_workspace_bytes(3, c + 1, 5) == 256 + 3 * 2 * 5 * 64
