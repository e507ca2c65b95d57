"""Device parity of the dense fronts (spicey_amd/csrc/fronts_exec.h) on the block circuits of tests/front_cases.py.

Most of fronts_exec.h exists twice: the host form the emulator runs (tests/test_front_paths.py holds these cases to the
oracle there) and the text under __HIP_DEVICE_COMPILE__ — the diagonal block in registers, the MFMA tile walks of
trailing / trailing_left / trailing_left_cols, the look-ahead, solve16, the root that stays in LDS — which only a device
runs.  tests/test_front_paths.py shows from the engine's own predicates that the cases hold every class of front: at the
LDS residency bound with several panels and a contribution block, staged by size with a second and third operand fetch of
the left-looking updates, too large for the left-looking sweep (the right-looking fallback with no knob set), U rows that
do not fit beside the solve's scratch, fewer and more tile columns than waves, staged fronts under staged and under
LDS-resident parents.

Every case runs on the one-workgroup kernel (force_global with one workgroup per instance: the executor that keeps no root
in LDS) and on groups of 2, as many workgroups as there are fronts, and more than that; interpreter=1 by itself is a group of
128 here, the plan's width for a workspace beyond LDS.  Threads: the plan's own 128 or 256 and the 512 of the full-size
mesh.  With the fronts placed by size and all staged
(stage_fronts); left-looking and with SPICEY_FRONT_RIGHT_LOOKING.  Every run: status 0, the oracle's iteration counts,
voltages, currents and end state within the project's bar (1e-9 relative + 1e-12), a handle that reports the CPU plan
and census — and within a case ALL runs give the same bits, which is what fronts_exec.h and the README promise across
G, placement and sweep.  No pair of variants had to be excepted from that."""
import numpy as np
import pytest

import front_cases as fc
from emul.pyemul import front_census
from spicey_amd import abi
from test_gpu_parity import tol_ratio

pytestmark = pytest.mark.gpu

CASES = list(fc.SHAPES)
_BITS: dict = {}  # case -> (variant, out_v, out_i, iters, state) of the first device run of the case in this process


def kernels(n_fronts):
    """The kernel / workgroup variants of one case."""
    return [dict(interpreter=1),  # (with a workspace beyond LDS the plan makes this a group as wide as the device allows)
            dict(force_global=True, wgs_per_inst=1),  # the one-workgroup kernel: no root kept in LDS
            dict(force_global=True, wgs_per_inst=2, threads=fc.THREADS),
            dict(force_global=True, wgs_per_inst=n_fronts),
            dict(force_global=True, wgs_per_inst=n_fronts + 3, threads=fc.THREADS)]  # idle workgroups; every front on its own


def plan_of(flat, kw, stage, profile=False):
    opts = {k: int(v) for k, v in kw.items()}
    return fc.cpu_plan(flat, front_cut=fc.FRONT_CUT, want_currents=1, profile=int(profile), debug=8 if stage else 0, **opts)


def check_info(info, flat, kw, stage, cen):
    plan = plan_of(flat, kw, stage)
    assert (info["n_fronts"], info["max_front"], info["front_cut"]) == (cen["n_fronts"], cen["max_front"], fc.FRONT_CUT), (kw, info)
    for k in ("wgs_per_inst", "lds_bytes", "threads", "interpreter", "inst_per_wg", "factor_reuse", "front_ws_bytes"):
        assert info[k] == plan[k], (kw, k, info[k], plan[k])
    assert info["factor_reuse"] == 0
    if "wgs_per_inst" in kw:
        assert info["wgs_per_inst"] == kw["wgs_per_inst"]


def check_against(got, ref, what):
    assert got["status"] == 0, (what, got["detail"])
    assert np.array_equal(got["iters"], ref["iters"]), what
    r = {"out_v": tol_ratio(got["out_v"], ref["out_v"]).max(), "out_i": tol_ratio(got["out_i"], ref["out_i"]).max(),
         "C_vprev": tol_ratio(got["state"]["C_vprev"], ref["state"]["C_vprev"]).max(),
         "D_vdprev": tol_ratio(got["state"]["D_vdprev"], ref["state"]["D_vdprev"]).max()}
    print("front-ratio", what, " ".join(f"{k}={v:.2e}" for k, v in r.items()))
    assert max(r.values()) <= 1.0, (what, r)


def same_bits(got, first, what):
    for k in ("out_v", "out_i", "iters"):
        assert np.array_equal(got[k], first[k]), (what, k)
    for k in ("C_vprev", "D_vdprev"):
        assert np.array_equal(got["state"][k], first["state"][k]), (what, k)


@pytest.mark.parametrize("stage", [False, True], ids=["by_size", "all_staged"])
@pytest.mark.parametrize("name", CASES)
def test_every_kernel_and_sweep_gives_the_oracles_answer_and_one_set_of_bits(name, stage, oracle_backend, monkeypatch):
    from spicey_amd.lib import HipBackend
    c = fc.case(name)
    ref = fc.oracle_ref(c, oracle_backend)
    cen = front_census(c.flat, fc.FRONT_CUT)
    for right in (False, True):
        if right:
            monkeypatch.setenv("SPICEY_FRONT_RIGHT_LOOKING", "1")  # (read when the handle is created)
        else:
            monkeypatch.delenv("SPICEY_FRONT_RIGHT_LOOKING", raising=False)
        for kw in kernels(cen["n_fronts"]):
            what = (name, "all staged" if stage else "by size", "right" if right else "left", tuple(kw.items()))
            be = HipBackend(front_cut=fc.FRONT_CUT, stage_fronts=stage, **kw)
            got = be.run(c.flat, c.steps, c.dt, c.src)
            check_against(got, ref, what)
            check_info(be.info, c.flat, kw, stage, cen)
            first = _BITS.setdefault(name, (what, got))
            same_bits(got, first[1], (what, "against", first[0]))


@pytest.mark.parametrize("name", CASES)
def test_a_profiled_run_reports_the_census_and_changes_no_bit(name):
    """Handle.front_ticks of a profiled run on two workgroups with every front staged: the fronts' pivots, boundary rows,
    parent and owning workgroup are the CPU census and schedule; the outputs are those of the unprofiled run."""
    from spicey_amd.lib import Handle
    c = fc.case(name)
    cen = front_census(c.flat, fc.FRONT_CUT, 2)
    kw = dict(force_global=True, wgs_per_inst=2, front_cut=fc.FRONT_CUT, stage_fronts=True)
    runs = {}
    for profile in (False, True):
        h = Handle(c.flat, profile=profile, **kw)
        try:
            runs[profile] = h.run(c.steps, c.dt, c.src)
            assert runs[profile]["status"] == 0, runs[profile]["detail"]
            if profile:
                ticks, meta = h.front_ticks()
                assert meta.shape == (cen["n_fronts"], 4) and ticks.shape == meta.shape
                for col, k in enumerate(("p", "q", "parent", "owner")):
                    assert np.array_equal(meta[:, col], cen[k]), (k, meta[:, col], cen[k])
                assert (ticks[:, 1] >= ticks[:, 0]).all() and (ticks[:, 3] >= ticks[:, 2]).all() and ticks[:, 3].min() > 0  # (assembled <= factored, solve begun <= done)
        finally:
            h.close()
    same_bits(runs[True], runs[False], name)
    if name in _BITS:
        same_bits(runs[False], _BITS[name][1], (name, "against", _BITS[name][0]))


def test_a_batch_of_distinct_instances_equals_the_solo_runs(oracle_backend):
    """Three instances of the three-level case with their own values, each on its own group of two workgroups with its own
    front workspace and flags, every front staged: each slot is its solo run bit for bit, and the oracle's answer."""
    from spicey_amd.lib import HipBackend
    cases = [fc.case("three_levels").reseeded(s) for s in (21, 22, 23)]
    flat, src = fc.batch_of(cases)
    kw = dict(force_global=True, wgs_per_inst=2, front_cut=fc.FRONT_CUT, stage_fronts=True)
    got = HipBackend(**kw).run(flat, cases[0].steps, cases[0].dt, src)
    assert got["status"] == 0, got["detail"]
    assert not np.array_equal(got["out_v"][0], got["out_v"][1]) and not np.array_equal(got["out_v"][1], got["out_v"][2])
    for i, c in enumerate(cases):
        solo = HipBackend(**kw).run(c.flat, c.steps, c.dt, c.src)
        check_against(solo, fc.oracle_ref(c, oracle_backend), ("solo", i))
        for k in ("out_v", "out_i", "iters"):
            assert np.array_equal(got[k][i], solo[k][0]), (i, k)
        for k in ("C_vprev", "D_vdprev"):
            assert np.array_equal(got["state"][k][i], solo["state"][k][0]), (i, k)


def test_a_second_run_continues_and_short_runs_end_right(oracle_backend):
    """A staged case (fronts placed by size: left-looking, six panels, under an LDS root): the second run of a handle starts
    from the state the first left — held to the oracle started from that very state —, and runs of no step and of one step
    give the first rows of the full run."""
    from spicey_amd.lib import Handle, HipBackend
    c = fc.case("wide_boundary")
    kw = dict(force_global=True, wgs_per_inst=2, front_cut=fc.FRONT_CUT)
    half = c.steps // 2
    h = Handle(c.flat, **kw)
    try:
        a = h.run(half, c.dt, c.src[: half + 1])
        b = h.run(c.steps - half, c.dt, c.src[half:])
    finally:
        h.close()
    assert a["status"] == 0 and b["status"] == 0, (a["detail"], b["detail"])
    ref_a = oracle_backend.run(c.flat, half, c.dt, c.src[: half + 1])
    check_against(a, ref_a, "first half")
    mid = c.flat.replicate(1)
    for k in ("C_vprev", "L_iprev", "D_vdprev", "S_ison"):
        getattr(mid, k)[...] = a["state"][k]
    ref_b = oracle_backend.run(mid, c.steps - half, c.dt, c.src[half:])
    check_against(b, ref_b, "second half, from the first one's state")
    assert not np.array_equal(a["out_v"][0, 0], b["out_v"][0, 0])  # (the second run really starts elsewhere)
    full = HipBackend(**kw).run(c.flat, c.steps, c.dt, c.src)
    assert full["status"] == 0
    for steps in (0, 1, half):
        short = HipBackend(**kw).run(c.flat, steps, c.dt, c.src[: steps + 1])
        assert short["status"] == 0, short["detail"]
        for k in ("out_v", "out_i", "iters"):
            assert short[k].shape[1] == steps + 1 and np.array_equal(short[k], full[k][:, : steps + 1]), (steps, k)
    for k in ("out_v", "out_i", "iters"):
        assert np.array_equal(a[k], full[k][:, : half + 1]), k


def test_a_floating_pair_in_a_staged_front_is_singular_and_the_batch_goes_on(oracle_backend, monkeypatch):
    """Singular through a staged multi-panel front (the late pivots of a six-panel front float): the oracle's status, from
    the left-looking sweep, the right-looking one and with every front staged; in a batch the instance is reported and the
    other two finish with the bits of their solo runs."""
    from spicey_amd.lib import Handle, HipBackend
    name, r = fc.FLOATING
    cases = [fc.case(name).reseeded(5, floating_pair=1e3), fc.case(name).reseeded(6, floating_pair=r), fc.case(name).reseeded(7, floating_pair=1e3)]
    want = [oracle_backend.run(c.flat, c.steps, c.dt, c.src)["status"] for c in cases]
    assert want == [0, abi.ERR_SINGULAR, 0]
    bad = cases[1]
    for right in (False, True):
        if right:
            monkeypatch.setenv("SPICEY_FRONT_RIGHT_LOOKING", "1")
        for kw in (dict(force_global=True, wgs_per_inst=1), dict(force_global=True, wgs_per_inst=2, stage_fronts=True)):
            got = HipBackend(front_cut=fc.FRONT_CUT, **kw).run(bad.flat, bad.steps, bad.dt, bad.src)
            assert got["status"] == want[1], (right, kw, got["status"], got["detail"])
    monkeypatch.delenv("SPICEY_FRONT_RIGHT_LOOKING", raising=False)
    flat, src = fc.batch_of(cases)
    kw = dict(force_global=True, wgs_per_inst=2, front_cut=fc.FRONT_CUT)
    h = Handle(flat, **kw)
    try:
        got = h.run(bad.steps, bad.dt, src)  # (one source table per instance: the instances that finish keep their results)
    finally:
        h.close()
    assert got["status"] == abi.ERR_SINGULAR and got["partial"] and list(got["inst_status"]) == want
    for i in (0, 2):
        solo = HipBackend(**kw).run(cases[i].flat, cases[i].steps, cases[i].dt, cases[i].src)
        assert solo["status"] == 0
        for k in ("out_v", "out_i", "iters"):
            assert np.array_equal(got[k][i], solo[k][0]), (i, k)
