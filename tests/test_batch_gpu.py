"""Per-instance source tables on the GPU (spicey_run_src, spicey_run_device_src, spicey_run_multi_src,
spicey_last_inst_status) in every plan, and simulateTRANBatch in both modes."""
import numpy as np
import pytest

from batch_variants import PerInstanceOracle, variant
from conftest import SMALL_GOLDENS, bits_equal, farr, golden_netlist, load_golden
from spicey_amd import abi, synth
from spicey_amd.netlist import parseNetlist
from spicey_amd.simulate import SingularMatrixError, simulateTRAN

pytestmark = pytest.mark.gpu


def tol_ratio(got, ref):
    return np.abs(np.asarray(got) - np.asarray(ref)) / (1e-9 * np.abs(np.asarray(ref)) + 1e-12)


def _amplitudes(src, n):
    """n distinct tables: the shared one scaled by 1, 0.9, 0.8, ... (the chains' source is a pulse from 0)."""
    return np.ascontiguousarray(np.stack([src * (1.0 - 0.1 * k) for k in range(n)]))


def _chain(n, ni, tran=".tran 1e-6 1.2e-5"):
    return synth.chain_batch("diode_chain", n, range(1, ni + 1), tran=tran)


def _mesh(rows, ni, tran=".tran 1e-6 6e-6"):
    ckt = parseNetlist(synth.rcd_mesh(rows, seed=5, tran=tran))
    dt, steps = abi.computeEffectiveTimeStep(ckt.analyses["tran"]["dt"], ckt.analyses["tran"]["tstop"])
    flat = abi.flatten(ckt).replicate(ni)
    flat.R_val *= np.linspace(1.0, 1.3, ni)[:, None]
    return flat, dt, steps, abi.source_table(ckt, dt, steps)


# (plan options, circuit, what SpiceyInfo must say)
PLANS = {
    "interp1": (dict(interpreter=1), lambda: _chain(40, 5), dict(interpreter=1)),
    "interp2_geom1": (dict(interpreter=2, geometry=1), lambda: _chain(700, 5), dict(interpreter=2, geometry=1)),
    "interp2_geom2": (dict(interpreter=2, geometry=2), lambda: _chain(700, 5), dict(interpreter=2, geometry=2)),
    "ipw1": (dict(inst_per_wg=1), lambda: _chain(40, 5), dict(inst_per_wg=1)),
    "ipw2": (dict(inst_per_wg=2), lambda: _chain(40, 5), dict(inst_per_wg=2)),
    "ipw4": (dict(inst_per_wg=4), lambda: _chain(40, 7), dict(inst_per_wg=4)),
    "force_global": (dict(force_global=True), lambda: _chain(40, 5), dict(lds_bytes=0)),
    "hybrid": (dict(), lambda: _chain(2600, 2, tran=".tran 1e-6 4e-6"), dict(interpreter=2)),
    "group": (dict(force_global=True, wgs_per_inst=4), lambda: _mesh(20, 2), dict(wgs_per_inst=4)),
    "interp3": (dict(interpreter=3), lambda: _chain(40, 5), dict(interpreter=3)),
}


def _run(kw, flat, steps, dt, src):
    from spicey_amd.lib import HipBackend
    be = HipBackend(**kw)
    res = be.run(flat, steps, dt, src)
    return res, be.info


@pytest.mark.parametrize("plan", sorted(PLANS))
def test_per_instance_tables_in_every_plan(plan):
    kw, make, expect = PLANS[plan]
    flat, dt, steps, src = make()
    tabs = _amplitudes(src, flat.n_inst)
    got, info = _run(kw, flat, steps, dt, tabs)
    assert got["status"] == 0, got["detail"]
    for k, v in expect.items():
        assert info[k] == v, (plan, k, info[k])
    if plan == "hybrid":
        assert info["hybrid_entries"] > 0
    assert (got["inst_status"] == 0).all()
    ref = PerInstanceOracle().run(flat, steps, dt, tabs)
    assert np.array_equal(got["iters"], ref["iters"])
    if kw.get("interpreter") == 3:
        assert bits_equal(got["out_v"], ref["out_v"]).all() and bits_equal(got["out_i"], ref["out_i"]).all()
        for k in ("C_vprev", "D_vdprev"):
            assert bits_equal(got["state"][k], ref["state"][k]).all()
    else:
        assert tol_ratio(got["out_v"], ref["out_v"]).max() <= 1.0 and tol_ratio(got["out_i"], ref["out_i"]).max() <= 1.0
        for k in ("C_vprev", "D_vdprev"):
            assert tol_ratio(got["state"][k], ref["state"][k]).max() <= 1.0
    # the instances really saw different tables
    assert not np.array_equal(got["out_v"][0], got["out_v"][1])
    # identical rows in the per-instance layout: the bits of the shared table
    same, _ = _run(kw, flat, steps, dt, np.ascontiguousarray(np.broadcast_to(src, tabs.shape)))
    shared, _ = _run(kw, flat, steps, dt, src)
    assert same["status"] == 0 and shared["status"] == 0
    for k in ("out_v", "out_i", "iters"):
        assert bits_equal(same[k], shared[k]).all() if k != "iters" else np.array_equal(same[k], shared[k]), (plan, k)


def test_switches_flip_at_different_steps_per_instance():
    """vswitch_pwl with one control PWL per instance (times stretched): the instances switch at different steps and each
    one's iteration counts are the oracle's."""
    texts = [variant(golden_netlist(load_golden("vswitch_pwl")), k, values=False, amplitude=False, pwl_times=True) for k in range(4)]
    ckts = [parseNetlist(t) for t in texts]
    dt, steps = abi.computeEffectiveTimeStep(ckts[0].analyses["tran"]["dt"], ckts[0].analyses["tran"]["tstop"])
    flat = abi.stack_instances([abi.flatten(c) for c in ckts])
    tabs = abi.source_tables(ckts, dt, steps)
    for kw in (dict(), dict(interpreter=3)):
        got, _ = _run(kw, flat, steps, dt, tabs)
        ref = PerInstanceOracle().run(flat, steps, dt, tabs)
        assert got["status"] == 0 and np.array_equal(got["iters"], ref["iters"])
        flips = [tuple(np.nonzero(ref["iters"][j] > 1)[0]) for j in range(4)]
        assert len(set(flips)) == 4 and all(flips)
        assert tol_ratio(got["out_v"], ref["out_v"]).max() <= 1.0


# torch initialises its HIP runtime first, as bench.py does, in a process of its own
_DEVICE_SRC = r"""
import sys
import numpy as np
import torch
dev = torch.device("cuda:0")
torch.zeros(1, device=dev)
sys.path[:0] = [sys.argv[1], sys.argv[1] + "/tests"]
from batch_variants import PerInstanceOracle
from spicey_amd import synth
from spicey_amd.lib import Handle
flat, dt, steps, src = synth.chain_batch("diode_chain", 40, range(1, 5), tran=".tran 1e-6 1.2e-5")
tabs = np.ascontiguousarray(np.stack([src * (1.0 - 0.1 * k) for k in range(4)]))
ref = PerInstanceOracle().run(flat, steps, dt, tabs)
d_src = torch.from_numpy(tabs).to(dev)
d_v = torch.zeros((4, steps + 1, flat.n_out), dtype=torch.float64, device=dev)
d_i = torch.zeros((4, steps + 1, flat.n_cur), dtype=torch.float64, device=dev)
d_it = torch.zeros((4, steps + 1), dtype=torch.int32, device=dev)
h = Handle(flat)
h.run_device(steps, dt, d_src.data_ptr(), d_v.data_ptr(), d_i.data_ptr(), d_it.data_ptr(), src_per_inst=True)
assert h.sync() == 0 and (h.inst_status() == 0).all()
tol = lambda g, r: (np.abs(g - r) / (1e-9 * np.abs(r) + 1e-12)).max()
assert np.array_equal(d_it.cpu().numpy(), ref["iters"])
assert tol(d_v.cpu().numpy(), ref["out_v"]) <= 1.0 and tol(d_i.cpu().numpy(), ref["out_i"]) <= 1.0
assert not np.array_equal(d_v[0].cpu().numpy(), d_v[1].cpu().numpy())
h.close()
print("device_src ok")
"""


def test_run_device_src_with_torch_tensors():
    import subprocess
    import sys
    from conftest import REPO
    r = subprocess.run([sys.executable, "-c", _DEVICE_SRC, REPO], capture_output=True, text=True, timeout=300, cwd=REPO)
    assert r.returncode == 0 and "device_src ok" in r.stdout, r.stdout + r.stderr


def test_run_multi_src_gives_each_shard_its_slice():
    from spicey_amd.lib import MultiHandle
    flat, dt, steps, src = _chain(40, 4)
    tabs = _amplitudes(src, 4)
    ref = PerInstanceOracle().run(flat, steps, dt, tabs)
    m = MultiHandle(flat, [0, 0])
    try:
        assert [s["n_inst"] for s in m.shards()] == [2, 2]
        got = m.run(steps, dt, tabs)
        assert got["status"] == 0 and np.array_equal(got["iters"], ref["iters"])
        assert tol_ratio(got["out_v"], ref["out_v"]).max() <= 1.0 and tol_ratio(got["out_i"], ref["out_i"]).max() <= 1.0
        shared = m.run(steps, dt, src)  # (continues from the first run's state: compare with the oracle's continuation)
        assert shared["status"] == 0
    finally:
        m.close()


def _near_sing_batch(n):
    """near_sing_b's topology n times; instance 1 is the singular original, the others ground node x through 1k .. nk."""
    bad = golden_netlist(load_golden("near_sing_b"))
    return [bad if j == 1 else bad.replace("1e16", f"{j + 1}k") for j in range(n)]


@pytest.mark.parametrize("kw,mates", [(dict(interpreter=3), ()), (dict(inst_per_wg=2), (0,)), (dict(inst_per_wg=4), (0, 2, 3))])
def test_last_inst_status_names_the_failing_instance(kw, mates):
    texts = _near_sing_batch(5)
    ckts = [parseNetlist(t) for t in texts]
    dt, steps = abi.computeEffectiveTimeStep(ckts[0].analyses["tran"]["dt"], ckts[0].analyses["tran"]["tstop"])
    flat = abi.stack_instances([abi.flatten(c) for c in ckts])
    got, info = _run(kw, flat, steps, dt, abi.source_tables(ckts, dt, steps))
    assert got["status"] == abi.ERR_SINGULAR and info["inst_per_wg"] == kw.get("inst_per_wg", 1)
    want = np.zeros(5, np.int32)
    want[1] = abi.ERR_SINGULAR
    want[list(mates)] = -1
    assert np.array_equal(got["inst_status"], want)
    ref = PerInstanceOracle().run(flat, steps, dt, abi.source_tables(ckts, dt, steps))
    for j in np.nonzero(want == 0)[0]:  # the instances that finished came back
        assert tol_ratio(got["out_v"][j], ref["out_v"][j]).max() <= 1.0
    # the batch front end runs the stopped mates again and returns every good circuit's result
    from spicey_amd.batch import simulateTRANBatch
    from spicey_amd.lib import HipBackend
    res = simulateTRANBatch([parseNetlist(t) for t in texts], backend=HipBackend(**kw))
    assert isinstance(res[1], SingularMatrixError)
    for j in (0, 2, 3, 4):
        solo = simulateTRAN(parseNetlist(texts[j]), backend=PerInstanceOracle())
        for k in solo["nodeVoltages"]:
            assert tol_ratio(res[j]["nodeVoltages"][k], solo["nodeVoltages"][k]).max() <= 1.0
        assert np.array_equal(res[j]["iterations"], solo["iterations"])


def _golden_texts():
    out = []
    for name in SMALL_GOLDENS + ["skip_quirk"]:
        text = golden_netlist(load_golden(name))
        out.append((name, text))
        out.append((name, text))  # a copy: the same topology, launched with the original
        out.append((None, variant(text, 1)))
    return out


def test_exact_batch_is_bit_equal_to_the_goldens():
    from spicey_amd.batch import simulateTRANBatch
    items = _golden_texts()
    ckts = [parseNetlist(t) for _, t in items]
    solo = [parseNetlist(t) for _, t in items]
    for ri in range(2):  # the second call continues from the state the first wrote
        got = simulateTRANBatch(ckts, exact_order=True)
        for i, ((name, _), g) in enumerate(zip(items, got)):
            if name is not None:
                run = load_golden(name)["runs"][ri] if ri < len(load_golden(name)["runs"]) else None
                if run is not None:
                    assert list(g["nodeVoltages"]) == run["keysV"] and list(g["elementCurrents"]) == run["keysI"]
                    assert g["times"] == run["times"]
                    for k in run["keysV"]:
                        assert bits_equal(g["nodeVoltages"][k], farr(run["V"][k])).all(), (name, ri, k)
                    for k in run["keysI"]:
                        assert bits_equal(g["elementCurrents"][k], farr(run["I"][k])).all(), (name, ri, k)
                    c = ckts[i]
                    assert [x.vPrev for x in c.C] == run["state"]["C_vPrev"] and [x.iPrev for x in c.L] == run["state"]["L_iPrev"]
                    assert [x.vdPrev for x in c.D] == run["state"]["D_vdPrev"] and [int(x.isOn) for x in c.S] == run["state"]["S_isOn"]
            # every slot, variants included: solo exact mode bit for bit (a variant may be singular where the original is not)
            try:
                ref = simulateTRAN(solo[i], exact_order=True)
            except SingularMatrixError:
                assert isinstance(g, SingularMatrixError), i
                continue
            assert list(g) == list(ref) and g["skipRisk"] == ref["skipRisk"] and np.array_equal(g["iterations"], ref["iterations"])
            for part in ("nodeVoltages", "elementCurrents"):
                assert list(g[part]) == list(ref[part])
                for k in g[part]:
                    assert bits_equal(g[part][k], ref[part][k]).all(), (i, ri, part, k)


def test_default_batch_meets_the_oracle():
    from spicey_amd.batch import simulateTRANBatch
    # (bridge_rectifier is ill-conditioned and skip_quirk is where the reference skips a row update: neither has a 1e-9 bar)
    # variants only of well-conditioned circuits: scaled values can make a near-singular or floating circuit ill-conditioned
    texts = [t for n, t in _golden_texts() if n is not None and n not in ("bridge_rectifier", "skip_quirk")]
    for name in ("two_probes", "transient01", "ladder20", "dchain20", "mesh6", "mesh9x5", "lc_tank", "star_hub"):
        texts += [variant(golden_netlist(load_golden(name)), k) for k in (1, 2)]
    texts += [variant(synth.diode_chain(60, seed=3, tran=".tran 1e-6 2e-5"), k) for k in range(6)]
    for diagnostics in (True, False):
        got = simulateTRANBatch([parseNetlist(t) for t in texts], diagnostics=diagnostics)
        for t, g in zip(texts, got):
            ref = simulateTRAN(parseNetlist(t), backend=PerInstanceOracle())
            assert list(g) == list(ref) and list(g["nodeVoltages"]) == list(ref["nodeVoltages"])
            assert list(g["elementCurrents"]) == list(ref["elementCurrents"]) and g["times"] == ref["times"]
            assert (g["skipRisk"] is None) == (not diagnostics)
            assert np.array_equal(g["iterations"], ref["iterations"])
            for k in ref["nodeVoltages"]:
                assert tol_ratio(g["nodeVoltages"][k], ref["nodeVoltages"][k]).max() <= 1.0, (t[:30], k)
            for k in ref["elementCurrents"]:
                assert tol_ratio(g["elementCurrents"][k], ref["elementCurrents"][k]).max() <= 1.0, (t[:30], k)


def _skip_island(val):
    """skip_quirk (nonzero skip counts in both modes) with an island x grounded through `val`: singular at 1e16 ohm
    (near_sing_b), solvable otherwise, one topology."""
    return golden_netlist(load_golden("skip_quirk")).replace(".tran", f"R9 x 0 {val}\n.tran")


@pytest.mark.parametrize("mode", ["exact", "default", "default_ipw2"])
def test_skip_risk_of_neighbours_of_a_singular_instance(mode):
    """A sweep with one singular corner: the instances that finished report their own skipRisk, as their solo runs do."""
    from spicey_amd.batch import simulateTRANBatch
    from spicey_amd.lib import HipBackend
    texts = [_skip_island("1k"), _skip_island("1e16"), variant(_skip_island("2.2k"), 1, values=False), _skip_island("3.3k")]
    exact = mode == "exact"
    solo = [None if i == 1 else simulateTRAN(parseNetlist(t), exact_order=exact) for i, t in enumerate(texts)]
    assert all(s["skipRisk"] > 0 for s in solo if s is not None)
    kw = dict(backend=HipBackend(diagnostics=1, inst_per_wg=2)) if mode == "default_ipw2" else dict(exact_order=exact)
    got = simulateTRANBatch([parseNetlist(t) for t in texts], **kw)
    assert isinstance(got[1], SingularMatrixError)
    for i in (0, 2, 3):
        assert got[i]["skipRisk"] == solo[i]["skipRisk"], (mode, i, got[i]["skipRisk"], solo[i]["skipRisk"])
        assert np.array_equal(got[i]["iterations"], solo[i]["iterations"])
        for k in solo[i]["nodeVoltages"]:
            if exact:
                assert bits_equal(got[i]["nodeVoltages"][k], solo[i]["nodeVoltages"][k]).all(), (i, k)
            else:
                assert tol_ratio(got[i]["nodeVoltages"][k], solo[i]["nodeVoltages"][k]).max() <= 1.0, (i, k)


def test_last_inst_status_needs_a_finished_run():
    import ctypes as C
    from spicey_amd.lib import Handle, SpiceyNativeError
    flat, dt, steps, src = _chain(40, 3)
    h = Handle(flat)
    try:
        st = np.zeros(3, np.int32)
        assert h.L.spicey_last_inst_status(h.h, st.ctypes.data_as(C.POINTER(C.c_int32))) == -1  # no run yet
        with pytest.raises(SpiceyNativeError):
            h.inst_status()
        assert h.run(steps, dt, _amplitudes(src, 3))["status"] == 0 and (h.inst_status() == 0).all()
        # a run refused before its launch: the previous run's answer does not stand for it
        assert h.L.spicey_run_src(h.h, steps, dt, src.ctypes.data_as(C.POINTER(C.c_double)), 7, None, None, None) == abi.ERR_BAD_DESC
        assert h.L.spicey_last_inst_status(h.h, st.ctypes.data_as(C.POINTER(C.c_int32))) == -1
    finally:
        h.close()
