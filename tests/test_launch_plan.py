"""spicey_create's launch plan (spicey_amd/csrc/launch_plan.cpp) without a device: the emulator library links the same
spicey_plan + fill_info as libspicey_hip.so.  Every selection rule is pinned here on a 256-CU device (MI355X); the
expectations are those of the rules as they stood when the plan moved out of spicey_create.  The GPU test at the end
checks that the library's handles report the plan the CPU computes."""
import ctypes as C
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from spicey_amd import abi, synth  # noqa: E402
from spicey_amd.netlist import parseNetlist  # noqa: E402

NCU = 256
_FLAT = {}


def _flat(ckt, n_inst):
    if ckt not in _FLAT:
        kind, n = ckt
        _FLAT[ckt] = abi.flatten(parseNetlist(getattr(synth, kind)(n)))
    f = _FLAT[ckt]
    return f.replicate(n_inst) if n_inst > 1 else f


def cpu_plan(ckt, n_inst=1, occupancy=1, **opts):
    from emul import pyemul
    d = _flat(ckt, n_inst).desc()
    o = abi.SpiceyOptions(**opts)
    info = abi.SpiceyInfo()
    err = C.create_string_buffer(256)
    rc = pyemul.lib().spicey_emul_plan(C.byref(d), C.byref(o), NCU, occupancy, C.byref(info), err, len(err))
    return rc, err.value.decode(), info.as_dict()


RC20, RC100, RC200, RC300, RC8000 = ("rc_ladder", 20), ("rc_ladder", 100), ("rc_ladder", 200), ("rc_ladder", 300), ("rc_ladder", 8000)
DC1000, DC2600, MESH20, MESH70 = ("diode_chain", 1000), ("diode_chain", 2600), ("rcd_mesh", 20), ("rcd_mesh", 70)

# (circuit, n_inst, options, expected SpiceyInfo fields)
CASES = {
    # v2: the smallest workgroup that holds the whole program in registers, 64 to 1024 threads
    "v2_64": (RC20, 1, {}, dict(interpreter=2, geometry=1, threads=64, inst_per_wg=1, resident_slots=28, tail_levels=10, lds_bytes=11888)),
    "v2_128": (RC100, 1, {}, dict(interpreter=2, geometry=1, threads=128, resident_slots=28, pcr_rows=63, lds_bytes=11184)),
    "v2_256": (RC200, 511, {}, dict(interpreter=2, geometry=1, threads=256, resident_slots=28, n_workgroups=511, lds_bytes=16752)),
    "v2_512": (RC300, 1, {}, dict(interpreter=2, geometry=1, threads=512, resident_slots=16, lds_bytes=22336)),
    "v2_1024": (DC1000, 1, {}, dict(interpreter=2, geometry=1, threads=1024, resident_slots=8, pcr_rows=64, lds_bytes=77456)),
    # packed geometry: automatic once n_inst >= 2 * #CU (and no explicit threads, no diagnostics), or asked for
    "packed_auto": (RC200, 512, {}, dict(interpreter=2, geometry=2, threads=512, resident_slots=4, n_workgroups=512)),
    "packed_not_below_2ncu": (RC200, 511, {}, dict(geometry=1, threads=256)),
    "packed_not_with_threads": (RC200, 512, dict(threads=512), dict(geometry=1, threads=512, resident_slots=16)),
    "packed_asked": (DC1000, 1, dict(geometry=2), dict(geometry=2, threads=512, resident_slots=4)),
    "packed_not_with_diagnostics": (RC200, 512, dict(diagnostics=1), dict(geometry=1, threads=256, resident_slots=28)),
    # hybrid workspace: 1024 threads by default, 512 on request
    "hybrid_1024": (DC2600, 1, {}, dict(interpreter=2, threads=1024, resident_slots=4, hybrid_entries=5118, lds_bytes=89264)),
    "hybrid_512": (DC2600, 1, dict(threads=512), dict(interpreter=2, threads=512, resident_slots=16, hybrid_entries=5118, lds_bytes=89264)),
    # global workspace: K = 2 from 2 * #CU instances, K = 4 from 4 * #CU (K <= 2 with diagnostics)
    "global_k2": (RC8000, 512, dict(force_global=1), dict(interpreter=1, inst_per_wg=2, n_workgroups=256, lds_bytes=0, wgs_per_inst=1, threads=1024)),
    "global_k4": (RC8000, 1024, dict(force_global=1), dict(interpreter=1, inst_per_wg=4, n_workgroups=256, lds_bytes=0, wgs_per_inst=1)),
    "global_k2_diagnostics": (RC8000, 1024, dict(force_global=1, diagnostics=1), dict(inst_per_wg=2, n_workgroups=512)),
    # group mode: G doubles while grid * G fits the CUs (16 without fronts, 128 with), G = 1 when the kernel cannot be resident
    "group_g16": (RC8000, 1, dict(force_global=1), dict(interpreter=1, wgs_per_inst=16, n_workgroups=1)),
    "group_g8": (RC8000, 20, dict(force_global=1), dict(wgs_per_inst=8, n_workgroups=20)),
    "group_occupancy_0": (RC8000, 1, dict(force_global=1, occupancy=0), dict(wgs_per_inst=1)),
    # dense fronts: automatic for a single large nonlinear instance, threads clamped to 512 (v1 would take 1024 here)
    "fronts_auto": (MESH20, 1, {}, dict(interpreter=1, threads=512, n_fronts=9, front_cut=10, wgs_per_inst=128, lds_bytes=0)),
    "fronts_clamp_512": (MESH70, 1, {}, dict(threads=512, n_fronts=119, wgs_per_inst=128)),
    "fronts_not_from_512_inst": (MESH20, 512, {}, dict(n_fronts=0, interpreter=2, threads=1024, tail_levels=24, n_workgroups=512)),
    "fronts_not_interleaved": (MESH20, 1, dict(inst_per_wg=2), dict(n_fronts=0, inst_per_wg=1, interpreter=2)),
    "fronts_never": (MESH20, 1, dict(front_cut=-1), dict(n_fronts=0, front_cut=0, interpreter=2)),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_plan_rules(name):
    ckt, n_inst, opts, want = CASES[name]
    opts = dict(opts)
    occupancy = opts.pop("occupancy", 1)
    rc, err, info = cpu_plan(ckt, n_inst, occupancy, **opts)
    assert rc == abi.OK, err
    assert {k: info[k] for k in want} == want


def test_no_hybrid_knob(monkeypatch):
    monkeypatch.setenv("SPICEY_NO_HYBRID", "1")
    rc, err, info = cpu_plan(DC2600)
    assert rc == abi.OK, err
    assert (info["hybrid_entries"], info["interpreter"], info["lds_bytes"], info["wgs_per_inst"], info["threads"]) == (0, 1, 0, 16, 512)


ERRORS = [
    (RC20, dict(inst_per_wg=3), abi.ERR_BAD_DESC, "inst_per_wg must be 0, 1, 2 or 4"),
    (RC20, dict(diagnostics=1, inst_per_wg=4), abi.ERR_BAD_DESC, "diagnostics need inst_per_wg <= 2 and geometry != 2"),
    (RC20, dict(diagnostics=1, geometry=2), abi.ERR_BAD_DESC, "diagnostics need inst_per_wg <= 2 and geometry != 2"),
    (RC20, dict(force_global=1, interpreter=2), abi.ERR_BAD_DESC, "interpreter 2 needs the LDS workspace, < 65536 workspace entries and inst_per_wg = 1"),
    (MESH20, dict(threads=1024), abi.ERR_BAD_DESC, "front_cut needs threads <= 512"),
    (RC20, dict(threads=100), abi.ERR_BAD_DESC, "threads must be a multiple of 64 in [64, 1024]"),
    (RC20, dict(threads=1024, geometry=2), abi.ERR_BAD_DESC, "geometry 2 needs inst_per_wg = 1, <= 80 KB of LDS per instance and <= 1024 unknowns"),
    (RC20, dict(geometry=3), abi.ERR_BAD_DESC, "geometry must be 0, 1 or 2"),
    (RC20, dict(force_global=1, wgs_per_inst=300), abi.ERR_BAD_DESC, "wgs_per_inst must be in [0, 256] (and inst_per_wg <= 2 with it)"),
    (RC8000, dict(force_global=1, wgs_per_inst=4, occupancy=0), abi.ERR_HIP,
     "wgs_per_inst: the group-mode kernel cannot be resident on this device (occupancy query says 0 workgroups per CU)"),
]


@pytest.mark.parametrize("case", range(len(ERRORS)))
def test_plan_refusals(case):
    ckt, opts, code, msg = ERRORS[case]
    opts = dict(opts)
    occupancy = opts.pop("occupancy", 1)
    rc, err, _ = cpu_plan(ckt, 1, occupancy, **opts)
    assert (rc, err) == (code, msg)


def test_plan_refuses_bad_descriptor():
    from emul import pyemul
    d = _flat(RC20, 1).desc()
    d.abi_version = 99
    err = C.create_string_buffer(256)
    rc = pyemul.lib().spicey_emul_plan(C.byref(d), None, NCU, 1, None, err, len(err))
    assert (rc, err.value.decode()) == (abi.ERR_BAD_DESC, "abi_version mismatch")


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["v2_64", "v2_1024", "packed_auto", "hybrid_1024", "global_k2", "group_g16", "fronts_auto"])
def test_handle_reports_the_cpu_plan(name):
    """libspicey_hip.so runs the policy this file pins: the handle's SpiceyInfo is the CPU plan's, field for field."""
    import torch
    from spicey_amd.lib import Handle
    assert torch.cuda.get_device_properties(0).multi_processor_count == NCU
    ckt, n_inst, opts, want = CASES[name]
    h = Handle(_flat(ckt, n_inst), **{k: v for k, v in opts.items() if k != "occupancy"})
    try:
        info = h.info()
    finally:
        h.close()
    assert {k: info[k] for k in want} == want
    rc, err, cpu = cpu_plan(ckt, n_inst, **opts)
    assert rc == abi.OK, err
    assert info == cpu
