"""The products of two signals on the CPU: spicey_amd/csrc/power_exec.h — the code the kernels of power.hip run — through
the harness of tests/power_host (an emulation of the kernels' lane and chunk mapping, behind the judge of power.h) against
reduce_reference_power, the numpy definition.  The ten order-free fields bit for bit; the three sums within the bound that
holds for any summation order: |err| <= (n + 1) 2^-52 sum |term| (n terms: n - 1 additions of relative error 2^-53 each
compound to less than n 2^-53, the products add one rounding; a factor 2 is left for the reference's own sum)."""
import os
import sys

import numpy as np
import pytest

from conftest import REPO, bits_equal
from spicey_amd.measure import make_power_reqs

sys.path.insert(0, os.path.join(REPO, "tests", "power_host"))
import pypower as pp  # noqa: E402

N_INST, N_I, DT = 3, 5, 1e-6


def n_points_list():
    c = pp.chunk()
    return [1, 2, c - 1, c, c + 1, 3 * c + 7]


@pytest.mark.parametrize("n_v", [1, 2, 65, 130])
def test_harness_equals_reference_and_a_request_stands_alone(n_v):
    c = pp.chunk()
    for n_points in n_points_list():
        out_v, out_i = pp.waveforms(N_INST, n_points, n_v, N_I, seed=1000 * n_v + n_points)
        pool = pp.request_pool(n_points, n_v, N_I, 300, seed=n_v + n_points)
        assert all((int(q["a_signal"]), int(q["b_signal"]), int(q["a_col_ref"]) >= 0, int(q["b_col_ref"]) >= 0, int(q["neg"])) == pp.combination(k)
                   for k, q in enumerate(pool))
        assert len({pp.combination(k) for k in range(len(pool))}) == 32
        assert len({q.tobytes() for q in pool}) < len(pool)  # (the same request more than once)
        zero_factor = [q for q in pool if (q["a_signal"] == 0 and q["a_col_ref"] == q["a_col"]) or (q["b_signal"] == 0 and q["b_col_ref"] == q["b_col"])]
        assert (len(zero_factor) > 0) == (n_v == 1)  # (a single column: v(x,x), a factor of exact zeros)
        assert any(q["step_from"] == q["step_to"] for q in pool)
        assert n_points <= 2 or any(q["step_from"] % c != 0 and q["step_to"] > q["step_from"] for q in pool)  # (a window that starts mid-chunk)
        assert n_points < 2 * c or any(q["step_from"] % c != 0 and q["step_to"] > q["step_from"] + c for q in pool)  # (and goes on through chunks of its own)
        full = pp.run(out_v, out_i, pool, DT)
        pp.check_against_reference(full, out_v, out_i, pool, DT)
        # a request's 16 doubles do not depend on the rest of the list: alone, and 65 of them in another order
        for k in (0, 1, 7, 150):
            assert bits_equal(pp.run(out_v, out_i, pool[k:k + 1], DT), full[:, k:k + 1]).all(), (n_points, k)
        perm = np.random.default_rng(n_v).permutation(300)[:65]
        assert bits_equal(pp.run(out_v, out_i, pool[perm], DT), full[:, perm]).all(), n_points
        # nor on the emulated launch: workgroup size and grid
        for threads, grid in ((64, 0), (1024, 0), (1, 0), (256, 1), (128, 3)):
            assert bits_equal(pp.run(out_v, out_i, pool[:65], DT, threads=threads, grid=grid), full[:, :65]).all(), (n_points, threads, grid)
        # nor on n_inst: an instance's samples alone, and among others
        assert bits_equal(pp.run(out_v[1:2], out_i[1:2], pool[:65], DT), full[1:2, :65]).all(), n_points
        more_v, more_i = np.concatenate([out_v[::-1], out_v, out_v[:1]]), np.concatenate([out_i[::-1], out_i, out_i[:1]])
        got = pp.run(more_v, more_i, pool[:65], DT)
        assert bits_equal(got[3:6], full[:, :65]).all() and bits_equal(got[6], full[0, :65]).all() and bits_equal(got[2], full[0, :65]).all(), n_points


def test_planted_ties_and_a_nan():
    c = pp.chunk()
    n_points = 3 * c + 7
    out_v, out_i = pp.waveforms(N_INST, n_points, 2, N_I, seed=5)
    v, i = out_v[0, :, 0], out_i[0, :, 1]
    p = v * i
    assert np.count_nonzero(p == p.min()) > 1 or np.count_nonzero(p == p.max()) > 1  # (ties occur by themselves)
    # the extremes planted twice: in two chunks, and on either side of a chunk edge — the first occurrence is reported
    v[[5, 2 * c + 3]], i[[5, 2 * c + 3]] = 3.0, 3.0
    v[[c - 1, c]], i[[c - 1, c]] = 3.0, -3.0
    req = make_power_reqs([(0, 0, -1, 1, 1, -1, 0, 0, -1), (0, 0, -1, 1, 1, -1, 1, 0, -1)])
    m = pp.run(out_v, out_i, req, DT)[0]
    assert (m[0][0], m[0][1], m[0][2], m[0][3]) == (-9.0, 9.0, float(c - 1), 5.0)
    assert (m[1][0], m[1][1], m[1][2], m[1][3]) == (-9.0, 9.0, 5.0, float(c - 1))  # (negated: the extremes change places)
    pp.check_against_reference(pp.run(out_v, out_i, req, DT), out_v, out_i, req, DT)
    # a NaN sample enters the sums and never replaces an extreme
    v[c + 9] = np.nan
    m = pp.run(out_v, out_i, req, DT)[0]
    ref = pp.reduce_reference_power(out_v, out_i, req, DT)[0]
    for r in range(2):
        assert np.isnan(m[r][4]) and np.isnan(m[r][7]) and not np.isnan(m[r][8])  # sum_p and sum_aa; b has no NaN
        assert bits_equal(m[r][pp.FREE], ref[r][pp.FREE]).all() and not np.isnan(m[r][pp.FREE]).any()
    assert (m[0][0], m[0][1], m[0][2], m[0][3]) == (-9.0, 9.0, float(c - 1), 5.0)
    # the other instances never saw it
    assert not np.isnan(pp.run(out_v, out_i, req, DT)[1:]).any()


OK = (0, 0, -1, 1, 0, -1, 0, 0, -1)


def _bad(field, value):
    q = make_power_reqs([OK, OK])
    q[1][field] = value
    return q


def test_refusals_one_per_clause():
    out_v, out_i = pp.waveforms(2, 10, 3, 2, seed=1)
    pp.run(out_v, out_i, make_power_reqs([OK]), DT)

    def refused(text, *a, **k):
        with pytest.raises(pp.Refused) as e:
            pp.run(*a, **k)
        assert str(e.value).startswith("power: ") and text in str(e.value), str(e.value)

    refused("unknown signal", out_v, out_i, _bad("a_signal", 2), DT)
    refused("unknown signal", out_v, out_i, _bad("b_signal", -1), DT)
    for field, value in (("a_col", 3), ("a_col", -1), ("a_col_ref", 3), ("a_col_ref", -2), ("b_col", 2), ("b_col", -1), ("b_col_ref", 2), ("b_col_ref", -2)):
        refused("column out of range", out_v, out_i, _bad(field, value), DT)
    refused("without a current buffer", out_v, None, make_power_reqs([OK]), DT)
    refused("column out of range", None, out_i, make_power_reqs([OK]), DT)  # (a voltage factor without a voltage buffer has no column)
    refused("neg must be 0 or 1", out_v, out_i, _bad("neg", 2), DT)
    refused("neg must be 0 or 1", out_v, out_i, _bad("neg", -1), DT)
    refused("reserved must be 0", out_v, out_i, _bad("reserved", 1), DT)
    for field, value in (("step_from", -1), ("step_to", 10), ("step_to", -2), ("step_from", 10)):
        refused("window outside", out_v, out_i, _bad(field, value), DT)
    q = _bad("step_from", 6)
    q[1]["step_to"] = 5
    refused("step_from > step_to", out_v, out_i, q, DT)
    for dt in (0.0, -1e-6, float("inf"), float("nan")):
        refused("dt must be finite and > 0", out_v, out_i, make_power_reqs([OK]), dt)
    L = pp.lib()
    need = L.spicey_power_host_workspace_bytes(2, 10, 1)
    refused("workspace of", out_v, out_i, make_power_reqs([OK]), DT, work_bytes=need - 1)
    pp.run(out_v, out_i, make_power_reqs([OK]), DT, work_bytes=need)
    refused("n_req must be >= 1", out_v, out_i, make_power_reqs([]), DT)
    refused("bad arguments", out_v, out_i, make_power_reqs([OK]), DT, have_out=False)
    refused("bad arguments", out_v, out_i, make_power_reqs([OK]), DT, n_inst=0)
    refused("n_points must be >= 1", out_v, out_i, make_power_reqs([OK]), DT, n_points=0)
    assert L.spicey_power_host_workspace_bytes(0, 10, 1) == -1 and L.spicey_power_host_workspace_bytes(1, 10, 0) == -1
    assert L.spicey_power_host_workspace_bytes(1, 0, 1) == -1
    c = pp.chunk()
    assert L.spicey_power_host_workspace_bytes(3, c + 1, 5) == 256 + 3 * 2 * 5 * 128
