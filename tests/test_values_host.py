"""The values pass on the CPU: spicey_amd/csrc/values_exec.h — the code the kernels of values.hip run — through the harness
of tests/values_host (an emulation of the kernels' lane and item mapping, behind the judge of values.h) against
reduce_reference_values, the numpy definition.  No field of a row is a sum, so every double is compared bit for bit."""
import os
import sys

import numpy as np
import pytest

from conftest import REPO, bits_equal
from spicey_amd import abi
from spicey_amd.measure import make_reqs, make_value_points, make_value_reqs, reduce_reference, reduce_reference_values, trace_buckets

sys.path.insert(0, os.path.join(REPO, "tests", "values_host"))
import pyvalues as pv  # noqa: E402

N_INST, N_I, DT, N_PTS = 3, 5, 1e-6, 40


def n_points_list():
    c = pv.chunk()
    return [2, 3, c - 1, c, c + 1, 3 * c + 7]


def case(n_v, n_points):
    out_v, out_i = pv.waveforms(N_INST, n_points, n_v, N_I, seed=1000 * n_v + n_points)
    pool = pv.request_pool(n_points, n_v, N_I, 300, seed=n_v + n_points, n_pts=N_PTS)
    return out_v, out_i, pool, pv.point_table(n_points, N_PTS, seed=n_points), pv.timing_rows(out_v, out_i, DT)


@pytest.mark.parametrize("n_v", [1, 2, 65, 130])
def test_harness_equals_reference_and_a_request_stands_alone(n_v):
    c = pv.chunk()
    for n_points in n_points_list():
        out_v, out_i, pool, pts, timing = case(n_v, n_points)
        kinds = pool["kind"]
        assert {(int(q["kind"]), int(q["signal"]), int(q["col_ref"]) >= 0) for q in pool} == {(k, s, r) for k in range(3) for s in range(2) for r in (False, True)}
        assert len({q.tobytes() for q in pool}) < len(pool)  # (the same request more than once)
        tr = pool[kinds == abi.VAL_TRACE]
        ns = np.where(tr["step_to"] == -1, n_points - 1, tr["step_to"]) - tr["step_from"] + 1
        assert (tr["buckets"] == ns).any() and (tr["buckets"] == 1).any()
        if n_points >= c - 1:
            assert {1, 2, 3, 7, 64, 65} <= set(tr["buckets"].tolist())
            assert ((tr["step_from"] % c != 0) & (ns > 1)).any()  # (a window that starts mid-chunk)
        if n_points >= 2 * c + 2:
            # buckets that end one before, on and one after their first sub-chunk's end
            assert {c - 1, c, c + 1} <= set(ns[tr["buckets"] == 1].tolist())
            assert {2 * c - 2, 2 * c - 1, 2 * c, 2 * c + 1, 2 * c + 2} <= set(ns[tr["buckets"] == 2].tolist())
        # the find rows: the pattern of found and not found is the numpy timing reference's; the planted level above the
        # maximum is never found, and where the run is long enough for three periods most of the others are
        found = timing[:, :, 3] >= 0
        assert not found[:, 3].any()
        if n_points >= c - 1:
            assert found.mean() >= 0.75, found
        else:
            assert not found.all()
        full = pv.run(out_v, out_i, pool, pts, DT, timing)
        ref = pv.check_against_reference(full, out_v, out_i, pool, pts, DT, timing)
        for r in np.nonzero(kinds == abi.VAL_FIND)[0]:
            t = int(pool[r]["timing_row"])
            assert ((full[:, r, 0] >= 0) == found[:, t]).all()
            hit = found[:, t]
            # (k + f) dt is the timing row's t_targ
            assert bits_equal((full[hit, r, 0] + full[hit, r, 1]) * DT, timing[hit, t, 4]).all(), (n_points, r)
            assert (full[~hit, r, :4] == [-1.0, 0.0, 0.0, 0.0]).all()
        assert ref.shape[2] == abi.val_row_doubles(pool)
        # a request's row does not depend on the rest of the list: alone, and 65 of them in another order
        stride = full.shape[2]
        for k in (0, 1, 2, 7, 150):
            assert bits_equal(pv.run(out_v, out_i, pool[k:k + 1], pts, DT, timing, out_stride=stride), full[:, k:k + 1]).all(), (n_points, k)
        perm = np.random.default_rng(n_v).permutation(300)[:65]
        assert bits_equal(pv.run(out_v, out_i, pool[perm], pts, DT, timing, out_stride=stride), full[:, perm]).all(), n_points
        # nor on the emulated launch: workgroup size and grid
        for threads, grid in ((64, 0), (1024, 0), (1, 0), (256, 1), (128, 3)):
            assert bits_equal(pv.run(out_v, out_i, pool[:65], pts, DT, timing, threads=threads, grid=grid, out_stride=stride), full[:, :65]).all(), (n_points, threads, grid)
        # nor on n_inst: an instance's samples alone, and among others
        assert bits_equal(pv.run(out_v[1:2], out_i[1:2], pool[:65], pts, DT, timing[1:2], out_stride=stride), full[1:2, :65]).all(), n_points
        more = [np.concatenate([a[::-1], a, a[:1]]) for a in (out_v, out_i, timing)]
        got = pv.run(more[0], more[1], pool[:65], pts, DT, more[2], out_stride=stride)
        assert bits_equal(got[3:6], full[:, :65]).all() and bits_equal(got[6], full[0, :65]).all() and bits_equal(got[2], full[0, :65]).all(), n_points


def test_properties_of_a_trace_and_of_points():
    c = pv.chunk()
    n_points = 3 * c + 7
    out_v, out_i = pv.waveforms(N_INST, n_points, 2, N_I, seed=11)
    for s0, s1 in ((0, n_points - 1), (c // 2 + 3, 2 * c + 150)):
        n = s1 - s0 + 1
        for B in (1, 2, 3, 7, 64, 65, n):
            req = make_value_reqs([(0, 1, 2, -1, 0, 0, -1, 0, s0, s1, 0, 0, B), (0, 0, 1, 0, 0, 0, -1, 0, s0, s1, 0, 0, B)])
            rows = pv.run(out_v, out_i, req, [], DT)
            lo, hi = trace_buckets(req[0])
            assert lo[0] == s0 and hi[-1] == s1 and (lo[1:] == hi[:-1] + 1).all() and (hi >= lo).all()
            for r, x in ((0, out_i[:, :, 2]), (1, out_v[:, :, 1] - out_v[:, :, 0])):
                b6 = rows[:, r, :6 * B].reshape(N_INST, B, 6)
                for b in range(B):
                    w = x[:, lo[b]:hi[b] + 1]
                    assert (b6[:, b, 0:1] <= w).all() and (w <= b6[:, b, 2:3]).all()  # min[b] <= x_s <= max[b]
                    assert bits_equal(b6[:, b, 4], w[:, 0]).all() and bits_equal(b6[:, b, 5], w[:, -1]).all()
                # the extremes over the buckets and their steps are stats' over the same window
                st = reduce_reference(out_v, out_i, make_reqs([(0, 1, 2, -1, s0, s1, 0.0, 0), (0, 0, 1, 0, s0, s1, 0.0, 0)]), DT)[:, r]
                for i in range(N_INST):
                    bmn, bmx = int(np.argmin(b6[i, :, 0])), int(np.argmax(b6[i, :, 2]))  # (first occurrence: the earlier bucket)
                    assert (b6[i, bmn, 0], b6[i, bmn, 1], b6[i, bmx, 2], b6[i, bmx, 3]) == (st[i, 0], st[i, 2], st[i, 1], st[i, 3])
                if B == n:  # the waveform itself, in every field
                    for j in (0, 2, 4, 5):
                        assert bits_equal(b6[:, :, j], x[:, s0:s1 + 1]).all()
                    assert (b6[:, :, 1] == np.arange(s0, s1 + 1)).all() and (b6[:, :, 3] == np.arange(s0, s1 + 1)).all()
    # points with f = 0 and f = 1 return the samples themselves
    k = np.arange(n_points - 1)
    pts = make_value_points([(int(a), 0.0) for a in k] + [(int(a), 1.0) for a in k])
    rows = pv.run(out_v, out_i, make_value_reqs([(1, 1, 3, -1, 0, 0, -1, 0, 0, 0, 0, len(pts), 0)]), pts, DT)[:, 0].reshape(N_INST, -1, 4)
    assert bits_equal(rows[:, :n_points - 1, 2], out_i[:, :-1, 3]).all() and bits_equal(rows[:, n_points - 1:, 2], out_i[:, 1:, 3]).all()
    assert bits_equal(rows[:, :n_points - 1, 3], (out_i[:, 1:, 3] - out_i[:, :-1, 3]) / DT).all()
    assert (rows[:, :, 0] == np.concatenate([k, k])).all() and (rows[:, :n_points - 1, 1] == 0.0).all() and (rows[:, n_points - 1:, 1] == 1.0).all()


def test_planted_ties_and_a_nan():
    c = pv.chunk()
    n_points = 3 * c + 7
    out_v, out_i = pv.waveforms(N_INST, n_points, 2, N_I, seed=5)
    v = out_v[0, :, 1]
    assert np.count_nonzero(v == v.min()) > 1 and np.count_nonzero(v == v.max()) > 1  # (ties occur by themselves)
    # the extremes planted twice in two sub-chunks of one bucket, and on either side of a bucket edge: the first is named
    v[[5, 2 * c + 3]] = 3.0
    v[[c + 40, 2 * c + 40]] = -3.0
    one = make_value_reqs([(0, 0, 1, -1, 0, 0, -1, 0, 0, -1, 0, 0, 1)])
    m = pv.run(out_v, out_i, one, [], DT)[0, 0]
    assert tuple(m[:6]) == (-3.0, float(c + 40), 3.0, 5.0, v[0], v[-1])
    two = make_value_reqs([(0, 0, 1, -1, 0, 0, -1, 0, 0, 2 * c + 5, 0, 0, 2)])  # buckets [0, c + 2] and [c + 3, 2c + 5]
    lo, hi = trace_buckets(two[0])
    assert (lo[1], hi[1]) == (c + 3, 2 * c + 5)
    v[[c + 2, c + 3]] = 4.0
    m = pv.run(out_v, out_i, two, [], DT)[0, 0]
    assert (m[2], m[3], m[8], m[9]) == (4.0, float(c + 2), 4.0, float(c + 3))
    for req in (one, two):
        pv.check_against_reference(pv.run(out_v, out_i, req, [], DT), out_v, out_i, req, [], DT, None)
    # a NaN sample never replaces an extreme ...
    v[c + 9] = np.nan
    m = pv.run(out_v, out_i, one, [], DT)[0, 0]
    assert tuple(m[:4]) == (-3.0, float(c + 40), 4.0, float(c + 2))
    # ... unless a sub-chunk of the bucket starts with it: then it is that sub-chunk's extreme and, as under stats, the
    # comparisons x < NaN and NaN < x never replace it or let it replace another
    v[c] = np.nan
    m = pv.run(out_v, out_i, one, [], DT)[0, 0]
    assert tuple(m[:4]) == (-3.0, float(2 * c + 40), 3.0, 5.0)  # (what the sub-chunk [c, 2c) held is behind its NaN)
    v[0] = np.nan
    m = pv.run(out_v, out_i, one, [], DT)
    assert np.isnan(m[0, 0, [0, 2, 4]]).all() and (m[0, 0, [1, 3]] == 0.0).all()
    pv.check_against_reference(m, out_v, out_i, one, [], DT, None)
    for B in (2, 7, n_points):
        req = make_value_reqs([(0, 0, 1, -1, 0, 0, -1, 0, 0, -1, 0, 0, B), (0, 0, 1, 0, 0, 0, -1, 0, 3, -1, 0, 0, min(B, n_points - 3))])
        pv.check_against_reference(pv.run(out_v, out_i, req, [], DT), out_v, out_i, req, [], DT, None)
    # the other instances never saw it
    assert not np.isnan(m[1:]).any()
    # a NaN bracketing a point shows in that point alone
    pts = make_value_points([(c + 8, 0.5), (c + 9, 0.0), (c + 10, 0.5)])
    req = make_value_reqs([(1, 0, 1, -1, 0, 0, -1, 0, 0, 0, 0, 3, 0)])
    got = pv.run(out_v, out_i, req, pts, DT)
    assert np.isnan(got[0, 0, [2, 3, 6, 7]]).all() and not np.isnan(got[0, 0, 8:]).any()
    pv.check_against_reference(got, out_v, out_i, req, pts, DT, None)


TRACE_OK = (0, 0, 0, -1, 0, 0, -1, 0, 0, -1, 0, 0, 4)
POINTS_OK = (1, 1, 0, -1, 0, 0, -1, 0, 0, 0, 0, 2, 0)
FIND_OK = (2, 0, 1, -1, 1, 0, -1, 0, 0, 0, 0, 0, 0)
PTS_OK = [(0, 0.0), (8, 1.0)]


def _bad(which, field, value):
    q = make_value_reqs([TRACE_OK, POINTS_OK, FIND_OK])
    q[which][field] = value
    return q


def test_refusals_one_per_clause():
    out_v, out_i = pv.waveforms(2, 10, 3, 2, seed=1)
    timing = np.full((2, 1, 8), -1.0)
    ok = make_value_reqs([TRACE_OK, POINTS_OK, FIND_OK])
    pv.run(out_v, out_i, ok, PTS_OK, DT, timing)

    def refused(text, *a, **k):
        with pytest.raises(pv.Refused) as e:
            pv.run(*a, **k)
        assert str(e.value).startswith("values: ") and text in str(e.value), str(e.value)

    refused("unknown kind", out_v, out_i, _bad(0, "kind", 3), PTS_OK, DT, timing)
    refused("unknown kind", out_v, out_i, _bad(0, "kind", -1), PTS_OK, DT, timing)
    refused("unknown signal", out_v, out_i, _bad(1, "signal", 2), PTS_OK, DT, timing)
    refused("unknown signal of the edge", out_v, out_i, _bad(2, "x_signal", -1), PTS_OK, DT, timing)
    for which, field, value in ((0, "col", 3), (0, "col", -1), (1, "col_ref", 2), (1, "col_ref", -2), (2, "col", 3)):
        refused("column out of range", out_v, out_i, _bad(which, field, value), PTS_OK, DT, timing)
    for field, value in (("x_col", 2), ("x_col", -1), ("x_col_ref", 2), ("x_col_ref", -2)):
        refused("column of the edge out of range", out_v, out_i, _bad(2, field, value), PTS_OK, DT, timing)
    refused("without a current buffer", out_v, None, ok[1:2], PTS_OK, DT, timing)
    refused("without a current buffer", out_v, None, ok[2:3], PTS_OK, DT, timing)  # (the edge's signal is a current)
    refused("column out of range", None, out_i, ok[:1], PTS_OK, DT, timing)  # (a voltage signal without a voltage buffer has no column)
    for field, value in (("step_from", -1), ("step_to", 10), ("step_to", -2), ("step_from", 10)):
        refused("window outside", out_v, out_i, _bad(0, field, value), PTS_OK, DT, timing)
    q = _bad(0, "step_from", 6)
    q[0]["step_to"] = 5
    refused("step_from > step_to", out_v, out_i, q, PTS_OK, DT, timing)
    for B in (0, -1, 11, pv.lib().spicey_values_host_max_buckets() + 1):
        refused("buckets outside", out_v, out_i, _bad(0, "buckets", B), PTS_OK, DT, timing)
    pv.run(out_v, out_i, _bad(0, "buckets", 10), PTS_OK, DT, timing)
    for field, value in (("first", -1), ("first", 3), ("count", 0), ("count", 3), ("count", -1)):
        refused("point run outside the table", out_v, out_i, _bad(1, field, value), PTS_OK, DT, timing)
    refused("point run outside the table", out_v, out_i, ok, [], DT, timing)
    for pt, text in (((-1, 0.5), "k outside"), ((9, 0.5), "k outside"), ((0, -0.25), "f outside"), ((0, 1.5), "f outside"), ((0, float("nan")), "f outside"),
                     ((0, float("inf")), "f outside")):
        refused("values: point 1: " + text, out_v, out_i, ok, [PTS_OK[0], pt], DT, timing)
    for which in (1, 2):
        refused("need n_points >= 2", out_v[:, :1], out_i[:, :1], ok[which:which + 1], [], DT, timing, n_pts=0)
    pv.run(out_v[:, :1], out_i[:, :1], make_value_reqs([TRACE_OK[:12] + (1,)]), [], DT)
    refused("timing_row outside", out_v, out_i, _bad(2, "timing_row", 1), PTS_OK, DT, timing)
    refused("timing_row outside", out_v, out_i, _bad(2, "timing_row", -1), PTS_OK, DT, timing)
    refused("without timing rows", out_v, out_i, ok, PTS_OK, DT, None)
    pv.run(out_v, out_i, ok[:2], PTS_OK, DT, None)
    refused("is shorter than the longest", out_v, out_i, ok, PTS_OK, DT, timing, out_stride=23)
    pv.run(out_v, out_i, ok, PTS_OK, DT, timing, out_stride=24)
    for dt in (0.0, -1e-6, float("inf"), float("nan")):
        refused("dt must be finite and > 0", out_v, out_i, ok, PTS_OK, dt, timing)
    need = pv.workspace_bytes(2, 10, ok, 2)
    refused("workspace of", out_v, out_i, ok, PTS_OK, DT, timing, work_bytes=need - 1)
    pv.run(out_v, out_i, ok, PTS_OK, DT, timing, work_bytes=need)
    refused("n_req must be >= 1", out_v, out_i, make_value_reqs([]), PTS_OK, DT, timing)
    refused("bad arguments", out_v, out_i, ok, PTS_OK, DT, timing, have_out=False)
    refused("bad arguments", out_v, out_i, ok, PTS_OK, DT, timing, n_inst=0)
    refused("n_points must be >= 1", out_v, out_i, ok, PTS_OK, DT, timing, n_points=0)
    refused("n_pts must be >= 0", out_v, out_i, ok, PTS_OK, DT, timing, n_pts=-1)
    for which in range(3):
        refused("reserved must be 0", out_v, out_i, _bad(which, "reserved", 1), PTS_OK, DT, timing)


def test_workspace_bytes_in_closed_form():
    c = pv.chunk()
    assert c == 256

    def al(b):
        return 256 * ((b + 255) // 256)
    ok = make_value_reqs([TRACE_OK, POINTS_OK, FIND_OK])
    assert pv.workspace_bytes(0, 10, ok, 2) == -1 and pv.workspace_bytes(1, 0, ok, 2) == -1 and pv.workspace_bytes(1, 10, ok[:0], 2) == -1
    assert pv.workspace_bytes(1, 10, ok, 1) == -1  # (the point run does not fit the table)
    # point table | trace table | points table, each rounded up to 256 bytes, then [n_inst][sum of B * S][6] doubles
    assert pv.workspace_bytes(2, 10, ok, 2) == 256 + 256 + 256 + 256 * ((2 * 4 * 1 * 48 + 255) // 256)
    assert pv.workspace_bytes(2, 10, ok[1:], 2) == 256 + 0 + 256 + 0
    n_points = 100 * c + 1

    def traces(count, B, s0=0, s1=-1):
        return make_value_reqs([TRACE_OK[:8] + (s0, s1, 0, 0, B)] * count)

    def partial_bytes(reqs):
        return pv.workspace_bytes(3, n_points, reqs, 0) - al(len(reqs) * 48)

    # B buckets of ceil(n / B) steps at most: S = ceil(ceil(n / B) / c) slots each
    for B, S in ((1, 101), (2, 51), (100, 2), (101, 1), (4096, 1)):
        assert partial_bytes(traces(1, B)) == al(3 * B * S * 48)
    # a short window costs its own samples, not the run's chunks; requests add up
    assert partial_bytes(traces(1, 1, 5, 5 + c - 1)) == 256 * ((3 * 1 * 48 + 255) // 256)
    assert partial_bytes(traces(7, 2, 5, 5 + 2 * c)) == 256 * ((3 * 7 * 2 * 2 * 48 + 255) // 256)
    # ... so the workspace does not grow with n_req x the chunks of the run: 1000 requests of one short bucket each stay
    # below ONE chunk row of the measurement pass's layout [n_inst][max_chunks][n_req][8] for the same list
    thousand = partial_bytes(traces(1000, 1, 0, c - 1))
    assert thousand == al(3 * 1000 * 48)
    assert thousand < 3 * 101 * 1000 * 64 // 50
    # and points and finds take no partials at all
    assert pv.workspace_bytes(3, n_points, make_value_reqs([POINTS_OK] * 9 + [FIND_OK] * 9), 2) == 256 + 0 + 256 * ((18 * 64 + 255) // 256)
