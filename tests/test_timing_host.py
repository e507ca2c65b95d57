"""The edge-timing pass on the CPU: spicey_amd/csrc/timing_exec.h — the code the kernels of timing.hip run — through the
harness of tests/timing_host (an emulation of the kernels' lane, tile and chunk mapping, the base windows through the
measurement pass's own stages) against reduce_reference_timing, the numpy definition.  Every field has one value in any
evaluation order, so every comparison is bit for bit: there is no tolerance in this file."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import REPO, bits_equal
from spicey_amd import abi
from spicey_amd.measure import make_timing_reqs, reduce_reference_timing

for _d in ("measure_host", "timing_host"):
    sys.path.insert(0, os.path.join(REPO, "tests", _d))
import pymeasure as pm  # noqa: E402
import pytiming as pt  # noqa: E402

N_INST, N_I, DT = 3, 5, 1e-6
N_VS = [1, 2, 63, 64, 65, 130]


def n_points_list():
    c = pt.chunk()
    return [2, c - 1, c, c + 1, 3 * c + 7]


def _case(n_v, n_points):
    out_v, out_i = pm.waveforms(N_INST, n_points, n_v, N_I, seed=1000 * n_v + n_points)  # (the nine quarter-spaced values)
    return out_v, out_i, pt.request_pool(n_points, n_v, N_I, 300, seed=n_v + n_points)


def E(col=0, level=0.0, dir=1, n=1, kind=0, base=(0, -1), signal=0, col_ref=-1):
    return (signal, col, col_ref, dir, n, kind, base[0], base[1], level)


def test_the_pool_finds_and_misses():
    """Before anything else, on reduce_reference_timing alone: the comparisons below are not comparisons of empty results.
    Over the pools of every shape, at least half of the (instance, request) rows find every edge they ask for and at least
    a tenth miss one (n_points = 2 has one interval and n_v = 1 has v(0,0) = 0 among its signals: those shapes mostly miss,
    which is why the count is taken over all of them); and the mix the pool promises is there."""
    found = total = 0
    for n_v in N_VS:
        for n_points in n_points_list():
            out_v, out_i, pool = _case(n_v, n_points)
            f = pt.found_every_edge(reduce_reference_timing(out_v, out_i, pool, DT), pool)
            found, total = found + int(f.sum()), total + f.size
            if n_points > 2 and n_v > 1:  # (a shape with intervals to choose from and no v(0,0): half on its own)
                assert 2 * int(f.sum()) >= f.size, (n_v, n_points, int(f.sum()), f.size)
            edges = [q[k] for q in pool for k in ("trig", "targ") if k == "targ" or q["has_trig"]]
            assert {int(e["signal"]) for e in edges} == {0, 1} and {int(e["dir"]) for e in edges} == {1, -1, 0}
            assert {int(e["level_kind"]) for e in edges} == {0, 1, 2} and {int(e["n"]) for e in edges} == {-3, -2, -1, 1, 2, 3, 4}
            assert any(int(e["col_ref"]) >= 0 for e in edges) and any(float(e["level"]) == 1.25 for e in edges)
            assert any(int(e["level_kind"]) and int(e["base_from"]) == int(e["base_to"]) for e in edges) or n_points == 2
            assert {(int(q["has_trig"]), int(q["targ_from_trig"])) for q in pool} == {(0, 0), (1, 0), (1, 1)}
            assert len({q.tobytes() for q in pool}) < len(pool)
            if n_points > 2:
                assert any(int(q["step_to"]) - int(q["step_from"]) == 1 for q in pool)
    print(f"rows that find every edge: {found} of {total}")
    assert 2 * found >= total and 10 * (total - found) >= total


@pytest.mark.parametrize("n_v", N_VS)
def test_harness_equals_reference_and_a_row_stands_alone(n_v):
    assert pt.chunk() == pm.chunk()  # (one chunking for every reduction)
    for n_points in n_points_list():
        out_v, out_i, pool = _case(n_v, n_points)
        full = pt.run(out_v, out_i, pool, DT)
        ref = reduce_reference_timing(out_v, out_i, pool, DT)
        assert bits_equal(full, ref).all(), (n_points, np.argwhere(~bits_equal(full, ref))[:4])
        # a request's row does not depend on the rest of the list: shorter lists, alone, 65 of them in another order
        for count in (1, 65):
            assert bits_equal(pt.run(out_v, out_i, pool[:count], DT), full[:, :count]).all(), (n_points, count)
        for k in (1, 7, 150):
            assert bits_equal(pt.run(out_v, out_i, pool[k:k + 1], DT), full[:, k:k + 1]).all(), (n_points, k)
        perm = np.random.default_rng(n_v).permutation(300)[:65]
        assert bits_equal(pt.run(out_v, out_i, pool[perm], DT), full[:, perm]).all(), n_points
        # nor on the emulated launch: workgroup size and grid
        for threads, grid in ((64, 0), (1024, 0), (1, 0), (256, 1), (128, 3), (32, 5)):
            assert bits_equal(pt.run(out_v, out_i, pool[:65], DT, threads=threads, grid=grid), full[:, :65]).all(), (n_points, threads, grid)
        # nor on n_inst: an instance's samples alone, and among others
        assert bits_equal(pt.run(out_v[1:2], out_i[1:2], pool[:65], DT), full[1:2, :65]).all(), n_points
        more_v, more_i = np.concatenate([out_v[::-1], out_v, out_v[:1]]), np.concatenate([out_i[::-1], out_i, out_i[:1]])
        got = pt.run(more_v, more_i, pool[:65], DT)
        assert bits_equal(got[3:6], full[:, :65]).all() and bits_equal(got[6], full[0, :65]).all() and bits_equal(got[2], full[0, :65]).all(), n_points
        assert pt.workspace_bytes(N_INST, n_points, pool) > 0


def _both(out_v, reqs, out_i=None):
    """Rows of the harness, which must be the reference's."""
    got = pt.run(out_v, out_i, reqs, DT)
    assert bits_equal(got, reduce_reference_timing(out_v, out_i, reqs, DT)).all()
    return got


def _wave(x):
    return np.ascontiguousarray(np.asarray(x, dtype=np.float64)[None, :, None])


def test_a_crossing_in_the_interval_that_leaves_chunk_0():
    c = pt.chunk()
    x = np.zeros(2 * c + 3)
    x[c:] = 1.0  # the one rise, in interval (c - 1, c): chunk 0's
    r = _both(_wave(x), make_timing_reqs([(0, -1, None, E(level=0.25), 0)]))[0, 0]
    assert (r[3], r[4], r[7]) == (c - 1, ((c - 1) + 0.25) * DT, 1.0)


def test_a_trig_in_the_last_interval_finds_the_targ_only_there():
    n = pt.chunk() + 40
    a, b, late = np.zeros(n), np.zeros(n), np.zeros(n)
    a[n - 1] = 1.0       # trig: rises in the window's last interval
    b[n - 1] = 1.0       # a targ in that same interval
    late[n - 2:] = 1.0   # a targ one interval earlier
    v = np.stack([a, b, late], axis=1)[None]
    r = _both(v, make_timing_reqs([(0, -1, E(0, 0.5), E(1, 0.5), 1), (0, -1, E(0, 0.5), E(2, 0.5), 1), (0, -1, E(0, 0.5), E(2, 0.5), 0)]))[0]
    assert (r[0, 0], r[0, 3], r[0, 7]) == (n - 2, n - 2, 1.0) and (r[1, 0], r[1, 3], r[1, 7]) == (n - 2, -1.0, 0.0) and r[2, 3] == n - 3


def test_a_targ_in_the_triggers_interval_with_an_earlier_time_is_selected():
    a, b = np.zeros(12), np.zeros(12)
    a[6:], b[6:] = 1.0, 4.0  # both rise in interval 5; through 0.5 the targ is there after 1/8 step, the trig after 1/2
    r = _both(np.stack([a, b], axis=1)[None], make_timing_reqs([(0, -1, E(0, 0.5), E(1, 0.5), 1)]))[0, 0]
    assert (r[0], r[3]) == (5.0, 5.0) and r[4] < r[1] and (r[1], r[4]) == (5.5 * DT, 5.125 * DT)


def _square(n, half=4):
    return np.array([1.0 if (s // half) % 2 else 0.0 for s in range(n)])


def test_n_one_beyond_the_count_is_not_found():
    x = _square(3 * pt.chunk())
    cnt = int(_both(_wave(x), make_timing_reqs([(0, -1, None, E(level=0.5), 0)]))[0, 0, 7])
    r = _both(_wave(x), make_timing_reqs([(0, -1, None, E(level=0.5, n=cnt), 0), (0, -1, None, E(level=0.5, n=cnt + 1), 0),
                                          (0, -1, None, E(level=0.5, n=-cnt), 0), (0, -1, None, E(level=0.5, n=-cnt - 1), 0)]))[0]
    assert cnt == 96 and [row[3] >= 0 for row in r] == [True, False, True, False] and (r[1, 4], r[1, 7]) == (-1.0, float(cnt))


def test_n_minus_one_equals_n_count():
    x = _square(3 * pt.chunk() + 5, half=7)
    r = _both(_wave(x), make_timing_reqs([(0, -1, None, E(level=0.5, dir=0, n=-1), 0)]))[0, 0]
    last = _both(_wave(x), make_timing_reqs([(0, -1, None, E(level=0.5, dir=0, n=int(r[7])), 0)]))[0, 0]
    assert r[7] > 100 and bits_equal(r, last).all()


def test_a_flat_signal_has_its_level_and_no_crossing():
    x = np.full(300, 2.5)
    r = _both(_wave(x), make_timing_reqs([(0, -1, None, E(level=0.5, dir=0, kind=1), 0), (0, -1, None, E(level=1.25, dir=0, kind=2), 0)]))[0]
    assert [(row[3], row[4], row[5], row[7]) for row in r] == [(-1.0, -1.0, 2.5, 0.0)] * 2


def test_the_same_edge_as_trig_and_targ():
    x = _square(600, half=5)
    e1, e2 = E(level=0.5, kind=1), E(level=0.5, kind=1, n=2)
    r = _both(_wave(x), make_timing_reqs([(0, -1, e1, e1, 1), (0, -1, e1, e2, 0), (0, -1, e1, e2, 1)]))[0]
    # from the trigger on, n = 1 is the trigger's own crossing; the period is n = 1 -> n = 2 under the default rule
    assert r[0, 3] == r[0, 0] == 4.0 and r[0, 4] == r[0, 1] and r[1, 3] - r[1, 0] == 10.0 and r[2, 3] == r[1, 3] and r[0, 7] == r[0, 6] == 60.0


def test_scaled_copies_have_scaled_levels_and_equal_times():
    out_v, _ = pm.waveforms(1, 2 * pt.chunk() + 9, 2, 1, seed=5)
    v = np.concatenate([out_v * s for s in (1.0, 2.0, 0.25, 8.0)])  # (powers of two: every product exact)
    reqs = make_timing_reqs([(0, -1, E(0, 0.5, kind=1, n=2), E(1, 0.25, kind=2, dir=0, n=-2, base=(3, 400)), 1), (5, 300, None, E(0, 0.75, kind=1, col_ref=1, dir=-1, n=3), 0)])
    r = _both(v, reqs)
    for i, s in enumerate((1.0, 2.0, 0.25, 8.0)):
        assert bits_equal(r[i][:, [0, 1, 3, 4, 6, 7]], r[0][:, [0, 1, 3, 4, 6, 7]]).all() and bits_equal(r[i][:, [2, 5]], r[0][:, [2, 5]] * s).all(), i
    assert (r[0][:, 3] >= 0).all() and r[0, 0, 0] >= 0


def test_workspace_bytes_and_refusals():
    out_v, out_i = pm.waveforms(2, 10, 3, 2, seed=1)
    ok = (0, -1, E(0, 0.5, kind=1), E(1, 0.25), 1)
    one = make_timing_reqs([ok])
    pt.run(out_v, out_i, one, DT)
    # 2 edges x 56 B -> 256 | 1 request x 16 B -> 256 | base rows 2 inst x 1 base x 64 B -> 256 | the measurement pass's
    # workspace for one base (its table 256 + 2 inst x 1 chunk x 64 B) -> 512 | counts 2 inst x 1 chunk x 2 edges x 4 B -> 256
    need = pt.workspace_bytes(2, 10, one)
    assert need == 256 + 256 + 256 + 512 + 256
    pt.run(out_v, out_i, one, DT, work_bytes=need)
    with pytest.raises(pt.Refused, match="timing"):
        pt.run(out_v, out_i, one, DT, work_bytes=need - 8)  # a short workspace
    assert pt.workspace_bytes(2, 10, make_timing_reqs([(0, -1, None, E(0, 0.5), 0)])) == 256 + 256 + 0 + 0 + 256  # (no base: no region for it)
    assert pt.workspace_bytes(0, 10, one) == -1 and pt.workspace_bytes(2, 0, one) == -1 and pt.workspace_bytes(2, 10, make_timing_reqs([])) == -1
    nan, inf = float("nan"), float("inf")
    bad_edges = [E(signal=2), E(signal=-1), E(dir=2), E(dir=-2), E(kind=3), E(kind=-1), E(n=0), E(level=nan), E(level=inf), E(level=-inf, kind=1),
                 E(kind=1, base=(-1, 5)), E(kind=1, base=(0, 10)), E(kind=2, base=(6, 5)), E(kind=1, base=(0, -2)), E(kind=2, base=(10, -1))]
    bad_cols = [E(col=3), E(col=-1), E(col_ref=3), E(col_ref=-2), E(signal=1, col=2)]  # n_v = 3, n_i = 2: only the buffers tell
    bad = [(0, -1, None, e, 0) for e in bad_edges] + [(0, -1, e, E(), 0) for e in bad_edges] + [
        (-1, 5, None, E(), 0), (0, 10, None, E(), 0), (6, 5, None, E(), 0), (0, -2, None, E(), 0),  # windows outside the run or reversed
        (5, 5, None, E(), 0), (9, -1, None, E(), 0)]  # one point: no interval
    for b in bad:
        with pytest.raises(pt.Refused, match="timing"):
            pt.run(out_v, out_i, make_timing_reqs([ok, b]), DT, fill=7.0)
        assert pt.workspace_bytes(2, 10, make_timing_reqs([ok, b])) == -1
    for b in [(0, -1, None, e, 0) for e in bad_cols] + [(0, -1, e, E(), 0) for e in bad_cols]:
        with pytest.raises(pt.Refused, match="timing"):
            pt.run(out_v, out_i, make_timing_reqs([ok, b]), DT, fill=7.0)
    for has_trig, from_trig in ((0, 1), (2, 0), (1, 2), (-1, 0)):  # targ_from_trig without has_trig; flags that are no flags
        r = make_timing_reqs([ok])
        r["has_trig"], r["targ_from_trig"] = has_trig, from_trig
        with pytest.raises(pt.Refused, match="timing"):
            pt.run(out_v, out_i, r, DT)
    pt.run(out_v, out_i, make_timing_reqs([(0, -1, None, E(kind=1, base=(4, 4), level=1.02), 0), (8, 9, None, E(signal=1, col=1, col_ref=0), 0)]), DT)  # accepted
    ignored = make_timing_reqs([(0, -1, None, E(), 0)])
    ignored["trig"]["signal"], ignored["trig"]["n"] = 9, 0  # (has_trig = 0: the trig is not read)
    ignored["targ"]["base_from"] = 99  # (an absolute level: the base window is not read)
    pt.run(out_v, out_i, ignored, DT)
    with pytest.raises(pt.Refused, match="timing"):
        pt.run(out_v, None, make_timing_reqs([(0, -1, None, E(signal=1), 0)]), DT)  # a current without a current buffer
    with pytest.raises(pt.Refused, match="timing"):
        pt.run(out_v, out_i, make_timing_reqs([]), DT)  # n_req = 0
    for dt in (0.0, -DT, nan, inf):
        with pytest.raises(pt.Refused, match="timing"):
            pt.run(out_v, out_i, one, dt)
    L = pt.lib()  # null buffers
    err = pt.C.create_string_buffer(256)
    out = np.zeros((2, 1, 8))
    assert L.spicey_tim_host_run(2, 10, DT, None, 3, None, 0, one.ctypes.data, 1, out.ctypes.data, -1, 256, 0, err, 256) == 2 and b"timing" in err.value
    assert L.spicey_tim_host_run(2, 10, DT, out_v.ctypes.data, 3, None, 0, one.ctypes.data, 1, None, -1, 256, 0, err, 256) == 2 and b"timing" in err.value
    assert L.spicey_tim_host_run(2, 10, DT, out_v.ctypes.data, 3, None, 0, None, 1, out.ctypes.data, -1, 256, 0, err, 256) == 2 and b"timing" in err.value


def test_library_workspace_bytes_equals_the_harness():
    """spicey_timing_workspace_bytes (the library, no device needed) against the harness's, on pools and refused lists."""
    from spicey_amd import lib
    for n_v, n_points in ((1, 2), (65, pt.chunk() + 1), (130, 3 * pt.chunk() + 7)):
        _, _, pool = _case(n_v, n_points)
        for reqs in (pool, pool[:1], pool[:65]):
            assert lib.timing_workspace_bytes(N_INST, n_points, reqs) == pt.workspace_bytes(N_INST, n_points, reqs) > 0
    assert lib.timing_workspace_bytes(0, 10, make_timing_reqs([(0, -1, None, E(), 0)])) == -1
    assert lib.timing_workspace_bytes(2, 10, make_timing_reqs([])) == -1 and lib.timing_workspace_bytes(2, 10, make_timing_reqs([(5, 5, None, E(), 0)])) == -1


def test_selftest_under_the_host_sanitizers():
    """tests/timing_host/selftest.cpp: the harness against a scan of its own, built with -fsanitize=address,undefined as a
    stand-alone program and run as a child process."""
    p = subprocess.run([pt.selftest_path()], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and "all groups agree" in p.stdout and "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr, p.stdout[-2000:] + p.stderr[-2000:]


def test_timing_req_dtype_is_the_compilers_layout(tmp_path):
    src = ["#include <stdio.h>", "#include <stddef.h>", f'#include "{REPO}/include/spicey_hip.h"', "int main(void){"]
    efields, rfields = list(abi.TIMING_EDGE_DTYPE.names), list(abi.TIMING_REQ_DTYPE.names)
    src += [f'  printf("e.{f} %zu\\n", offsetof(SpiceyTimingEdge, {f}));' for f in efields]
    src += [f'  printf("r.{f} %zu\\n", offsetof(SpiceyTimingReq, {f}));' for f in rfields]
    src += ['  printf("e.__size %zu\\n", sizeof(SpiceyTimingEdge));', '  printf("r.__size %zu\\n", sizeof(SpiceyTimingReq));', "  return 0; }"]
    c = tmp_path / "timing_req.c"
    c.write_text("\n".join(src))
    exe = tmp_path / "timing_req"
    subprocess.run(["gcc", "-o", str(exe), str(c)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout
    got = {k: int(v) for k, v in (line.split() for line in out.strip().splitlines())}
    assert got.pop("e.__size") == abi.TIMING_EDGE_DTYPE.itemsize == 48 and got.pop("r.__size") == abi.TIMING_REQ_DTYPE.itemsize == 120
    want = {f"e.{f}": abi.TIMING_EDGE_DTYPE.fields[f][1] for f in efields}
    want.update({f"r.{f}": abi.TIMING_REQ_DTYPE.fields[f][1] for f in rfields})
    assert got == want
    assert {f"e.{f}": getattr(abi.SpiceyTimingEdge, f).offset for f in efields} == {k: v for k, v in got.items() if k[0] == "e"}
    assert {f"r.{f}": getattr(abi.SpiceyTimingReq, f).offset for f in rfields} == {k: v for k, v in got.items() if k[0] == "r"}
