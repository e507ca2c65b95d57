"""The spectrum pass on the CPU: the harness of tests/spectrum_host — spectrum_exec.h, the kernel's own arithmetic and
workgroup mapping — against reduce_reference_spectrum bit for bit, the independence of a row from the list, the instance
count and the emulated launch, a long-double DFT under the a-priori bound of the radix-2 FFT, the exact cases of the
rectangular window, and the judge's refusals."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import REPO
from spicey_amd import abi
from spicey_amd.measure import make_spec_reqs, reduce_reference_spectrum, spectrum_tables

sys.path.insert(0, os.path.join(REPO, "tests", "spectrum_host"))
import pyspectrum as ps  # noqa: E402

bits_equal = ps.bits_equal
N_POINTS = (1 << max(ps.LOG2NS)) + 3  # the longest N of the list + 3


@pytest.fixture(scope="module", params=ps.N_VS)
def case(request):
    """One run, its mixed request list and the harness's rows: computed once, read by every test below."""
    n_v = request.param
    out_v, out_i = ps.waveforms(ps.N_INST, N_POINTS, n_v, ps.N_I, seed=100 + n_v)
    pool = ps.request_pool(N_POINTS, n_v, ps.N_I, seed=n_v)
    full = ps.run(out_v, out_i, pool)
    for a in (out_v, out_i, full):
        a.setflags(write=False)
    return n_v, out_v, out_i, pool, full


def test_the_pool_covers_what_it_should(case):
    _, _, _, pool, _ = case
    assert set(pool["log2n"]) == set(ps.LOG2NS) and set(pool["window"]) == {0, 1} and set(pool["kind"]) == {0, 1} and set(pool["signal"]) == {0, 1}
    assert (pool["col_ref"] >= 0).any() and len({q.tobytes() for q in pool}) < len(pool)  # (repeated requests)
    assert set(pool["step_from"][pool["log2n"] == max(ps.LOG2NS)]) == {0, 3}
    for log2n in ps.LOG2NS:
        mine = pool[pool["log2n"] == log2n]
        assert {(int(q["bin_from"]), int(q["bin_to"])) for q in mine} == set(ps.bands(log2n))
    # N/2 butterflies of a stage against the wave (64) and the workgroup (256)
    assert [(1 << l) // 2 for l in ps.LOG2NS] == [4, 32, 64, 128, 256, 512, 1024]


def test_harness_equals_the_numpy_reference_bit_for_bit(case):
    _, out_v, out_i, pool, full = case
    ref = reduce_reference_spectrum(out_v, out_i, pool, ps.DT)
    assert full.shape == ref.shape == (ps.N_INST, len(pool), 2 * ((1 << max(ps.LOG2NS)) // 2 + 1))
    assert bits_equal(full, ref).all()
    for r, q in enumerate(pool):  # a row behind the request's own doubles is +0.0
        assert (full[:, r, ps.own_width(q):].view(np.int64) == 0).all(), r
    assert not np.isnan(full).any()


@pytest.mark.parametrize("log2n", ps.LOG2NS)
def test_a_run_of_n_plus_3_points(log2n):
    """n_points = N + 3, first steps 0 and 3: the last request ends on the run's last sample."""
    N = 1 << log2n
    for n_v in ps.N_VS:
        out_v, out_i = ps.waveforms(ps.N_INST, N + 3, n_v, ps.N_I, seed=7 * log2n + n_v)
        pool = ps.request_pool(N + 3, n_v, ps.N_I, seed=log2n, log2ns=(log2n,))
        assert set(pool["step_from"]) == {0, 3}
        got = ps.run(out_v, out_i, pool)
        assert bits_equal(got, reduce_reference_spectrum(out_v, out_i, pool, ps.DT)).all(), n_v
        # the samples outside a request's N do not enter it
        ov2 = out_v.copy()
        ov2[:, :3] += 1.0
        late = pool["step_from"] == 3
        assert bits_equal(ps.run(ov2, out_i, pool[late]), got[:, late, :ps.width(pool[late])]).all()


def test_a_row_does_not_depend_on_the_list_the_instances_or_the_launch(case):
    n_v, out_v, out_i, pool, full = case
    perm = np.random.default_rng(n_v).permutation(len(pool))[:17]
    sub = ps.run(out_v, out_i, pool[perm])
    assert bits_equal(sub, full[:, perm, :sub.shape[2]]).all()
    for r in (0, len(pool) // 2, len(pool) - 1):
        one = ps.run(out_v, out_i, pool[r:r + 1])
        assert bits_equal(one, full[:, r:r + 1, :one.shape[2]]).all(), r
    assert bits_equal(ps.run(out_v[1:2], out_i[1:2], pool), full[1:2]).all()  # another n_inst
    for threads, grid in ((64, 0), (1, 3), (1024, 1), (32, 7)):  # another workgroup size, workgroups that take several items
        assert bits_equal(ps.run(out_v, out_i, pool, threads=threads, grid=grid), full).all(), (threads, grid)


def test_tables_are_the_definition():
    for log2n in (3, 4, 10, 13):
        N = 1 << log2n
        T, w = ps.tables(log2n)
        t_re, t_im, w_py = spectrum_tables(log2n)
        assert bits_equal(T.real, t_re).all() and bits_equal(T.imag, t_im).all() and bits_equal(w, w_py).all()
        assert T[0] == 1.0 and T[N // 4] == -1j and w[0] == 0.0 and w[N // 2] == 1.0
        assert ps.twiddle_error(log2n) <= 8 * ps.U  # (a libm within a few ulps)
        assert ps.lds_bytes(log2n) == 16 * N
    assert ps.lds_bytes(13) == 128 * 1024


def test_accuracy_against_a_long_double_dft(case):
    """|err_k| <= t eta / (1 - t eta) sqrt(N) ||y||_2 (pyspectrum.dft_bound: Higham Thm 24.2 with the measured mu), no slack,
    for every bin of every request with N <= 1024: Gaussian columns and off-bin tones with an offset."""
    _, out_v, out_i, pool, full = case
    worst = ps.check_against_dft(full, out_v, out_i, pool, max_log2n=10)
    print(f"largest error / bound: {worst:.4f}")
    assert 0.0 < worst <= 1.0


def test_exact_cases_of_the_rectangular_window():
    ni, n_points = 2, 70
    for log2n in (3, 6):
        N = 1 << log2n
        half = N // 2
        full_band = make_spec_reqs([(0, 0, -1, 0, 3, log2n, 0, 0, half), (0, 0, -1, 1, 3, log2n, 0, 0, half), (0, 0, -1, 1, 3, log2n, 0, 1, half)])
        # an impulse at the window's first sample: every bin exactly (x0, 0)
        v = np.zeros((ni, n_points, 1))
        v[0, 3, 0], v[1, 3, 0] = 0.3, -1.7
        got = ps.run(v, None, full_band)
        for i, x0 in enumerate((0.3, -1.7)):
            assert (got[i, 0, 0:N + 2:2] == x0).all() and (got[i, 0, 1:N + 2:2] == 0.0).all()
            # all bins have the same power: the first of the band wins, and a neighbour that does not exist is -1.0
            assert got[i, 1, :6].tolist() == [0.0, x0, 0.0, -1.0, x0 * x0, x0 * x0] and got[i, 2, :6].tolist() == [1.0, x0, 0.0, x0 * x0, x0 * x0, x0 * x0]
        # the constant 0.25: bin 0 exactly (N / 4, 0), nothing else
        v = np.full((ni, n_points, 1), 0.25)
        got = ps.run(v, None, full_band)
        assert (got[:, 0, 0] == N / 4).all() and (got[:, 0, 1:N + 2] == 0.0).all()
        assert (got[:, 1, 0] == 0.0).all() and (got[:, 1, 4] == (N / 4) ** 2).all() and (got[:, 2, 0] == -1.0).all()
        # all zeros: all zeros, and no dominant bin
        got = ps.run(np.zeros((ni, n_points, 1)), None, full_band)
        assert (got[:, 0] == 0.0).all() and (got[:, 1:, 0] == -1.0).all() and (got[:, 1:, 1:] == 0.0).all()
        # two equal largest bins: 1 + (-1)^j has DC and Nyquist of power N^2 each (integers: exact) -> the lower one
        v = np.zeros((ni, n_points, 1))
        v[:, 3:3 + N, 0] = 1.0 + np.where(np.arange(N) % 2 == 0, 1.0, -1.0)
        q = make_spec_reqs([(0, 0, -1, 1, 3, log2n, 0, 0, half), (0, 0, -1, 1, 3, log2n, 0, 1, half), (0, 0, -1, 0, 3, log2n, 0, 0, half)])
        got = ps.run(v, None, q)
        assert (got[:, 2, 0] == N).all() and (got[:, 2, N] == N).all()  # (re of bin 0 and of bin N/2)
        assert (got[:, 0, 0] == 0.0).all() and (got[:, 0, 4] == float(N * N)).all()
        assert (got[:, 1, 0] == half).all() and (got[:, 1, 4] == float(N * N)).all() and (got[:, 1, 5] == -1.0).all()
    # a NaN sample makes every bin NaN: no bin wins
    v = np.ones((1, 16, 1))
    v[0, 5, 0] = np.nan
    got = ps.run(v, None, make_spec_reqs([(0, 0, -1, 1, 0, 3, 1, 0, 4)]))
    assert got[0, 0].tolist() == [-1.0, 0, 0, 0, 0, 0, 0, 0]
    assert bits_equal(got, reduce_reference_spectrum(v, None, make_spec_reqs([(0, 0, -1, 1, 0, 3, 1, 0, 4)]), ps.DT)).all()


def test_refusals_of_the_judge():
    out_v, out_i = ps.waveforms(2, 20, 3, 2, seed=1)
    ok = (0, 0, -1, 0, 0, 4, 1, 0, 8)  # N = 16
    bad = [(2, 0, -1, 0, 0, 4, 1, 0, 8), (-1, 0, -1, 0, 0, 4, 1, 0, 8),  # signal
           (0, 0, -1, 2, 0, 4, 1, 0, 8), (0, 0, -1, -1, 0, 4, 1, 0, 8),  # kind
           (0, 0, -1, 0, 0, 4, 2, 0, 8), (0, 0, -1, 0, 0, 4, -1, 0, 8),  # window
           (0, 3, -1, 0, 0, 4, 1, 0, 8), (0, -1, -1, 0, 0, 4, 1, 0, 8), (0, 0, 3, 0, 0, 4, 1, 0, 8), (0, 0, -2, 0, 0, 4, 1, 0, 8), (1, 2, -1, 0, 0, 4, 1, 0, 8),  # columns
           (0, 0, -1, 0, 0, 2, 1, 0, 2), (0, 0, -1, 0, 0, 14, 1, 0, 8), (0, 0, -1, 0, 0, 40, 1, 0, 8), (0, 0, -1, 0, 0, -1, 1, 0, 0),  # log2n
           (0, 0, -1, 0, -1, 4, 1, 0, 8), (0, 0, -1, 0, 5, 4, 1, 0, 8), (0, 0, -1, 0, 2 ** 62, 4, 1, 0, 8),  # first step
           (0, 0, -1, 0, 0, 4, 1, -1, 8), (0, 0, -1, 0, 0, 4, 1, 0, 9), (0, 0, -1, 0, 0, 4, 1, 5, 4)]  # band
    need = ps.workspace_bytes(2, 20, make_spec_reqs([ok]))
    assert need == 256 + 256 + 256  # (table | order | 16 twiddle doubles + 16 window doubles), each aligned
    cases = [(out_i, make_spec_reqs([ok, b]), 18, 4096, ps.DT) for b in bad]
    cases.append((None, make_spec_reqs([(1, 0, -1, 0, 0, 4, 1, 0, 8)]), 18, 4096, ps.DT))  # signal = 1 without a current buffer
    cases.append((out_i, make_spec_reqs([]), 18, 4096, ps.DT))  # n_req = 0
    cases.append((out_i, make_spec_reqs([ok]), 17, need, ps.DT))  # a row shorter than the band
    cases.append((out_i, make_spec_reqs([(0, 0, -1, 1, 0, 4, 1, 0, 0)]), 7, need, ps.DT))  # ... than a dominant's 8
    cases.append((out_i, make_spec_reqs([ok]), 18, need - 8, ps.DT))  # workspace too small
    cases += [(out_i, make_spec_reqs([ok]), 18, need, dt) for dt in (0.0, -1e-6, float("inf"), float("nan"))]
    for oi, reqs, stride, wb, dt in cases:
        with pytest.raises(ps.Refused, match="spectrum"):
            ps.run(out_v, oi, reqs, dt=dt, out_stride=stride, work_bytes=wb, fill=7.0)
    assert ps.workspace_bytes(0, 20, make_spec_reqs([ok])) == -1 and ps.workspace_bytes(2, 20, make_spec_reqs([bad[16]])) == -1
    assert ps.workspace_bytes(2, 20, make_spec_reqs([])) == -1
    # the accepted neighbours: the last N samples of the run, and a wider row whose tail is zero
    got = ps.run(out_v, out_i, make_spec_reqs([ok, (0, 0, -1, 1, 4, 4, 0, 8, 8)]), out_stride=21, work_bytes=need, fill=7.0)
    assert (got[:, 0, 18:].view(np.int64) == 0).all() and (got[:, 1, 8:].view(np.int64) == 0).all() and (got[:, :, :8] != 7.0).all()


def test_spec_req_dtype_is_the_compilers_layout(tmp_path):
    fields = list(abi.SPEC_REQ_DTYPE.names)
    src = ["#include <stdio.h>", "#include <stddef.h>", f'#include "{REPO}/include/spicey_hip.h"', "int main(void){"]
    src += [f'  printf("{f} %zu\\n", offsetof(SpiceySpecReq, {f}));' for f in fields]
    src += ['  printf("__size %zu\\n", sizeof(SpiceySpecReq));', '  printf("__min %d\\n", SPICEY_SPEC_MIN_LOG2N);', '  printf("__max %d\\n", SPICEY_SPEC_MAX_LOG2N);',
            "  return 0; }"]
    c = tmp_path / "spec_req.c"
    c.write_text("\n".join(src))
    exe = tmp_path / "spec_req"
    subprocess.run(["gcc", "-o", str(exe), str(c)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout
    got = {k: int(v) for k, v in (line.split() for line in out.strip().splitlines())}
    assert got.pop("__size") == abi.SPEC_REQ_DTYPE.itemsize == 40 and (got.pop("__min"), got.pop("__max")) == (abi.SPEC_MIN_LOG2N, abi.SPEC_MAX_LOG2N)
    assert got == {f: abi.SPEC_REQ_DTYPE.fields[f][1] for f in fields}
    import ctypes
    assert {f: getattr(abi.SpiceySpecReq, f).offset for f in fields} == got and ctypes.sizeof(abi.SpiceySpecReq) == 40
