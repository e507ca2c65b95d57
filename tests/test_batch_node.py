"""ts/simulateTRANBatch.ts executed under Node (the N-API stand-in for bun:ffi, tests/test_ts_dropin_node.py) on the GPU:
in exact mode every slot equals the Python batch and the reference-generated golden bit for bit."""
import json
import os
import shutil
import subprocess

import pytest

from batch_variants import variant
from conftest import REPO, bits_equal, farr, golden_netlist, load_golden
from spicey_amd.netlist import parseNetlist

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(shutil.which("node") is None, reason="node not available")]


def test_ts_batch_matches_python_and_goldens_in_exact_mode(tmp_path):
    from spicey_amd.batch import simulateTRANBatch
    from test_ts_dropin_node import NODE, _circuit_json, _prepare
    erased, libpath = _prepare(tmp_path)
    names = ["two_probes", "vswitch_pwl", "dchain20", "skip_quirk", "bridge_rectifier"]
    items = []
    for n in names:
        text = golden_netlist(load_golden(n))
        items += [(n, text), (n, text), (None, variant(text, 1))]
    items.append((None, golden_netlist(load_golden("err_singular"))))
    items.append((None, "* no tran\nV1 a 0 DC 1\nR1 a 0 1k\n.end\n"))
    cj, oj = str(tmp_path / "ckts.json"), str(tmp_path / "out.json")
    json.dump([_circuit_json(parseNetlist(t)) for _, t in items], open(cj, "w"))
    r = subprocess.run(NODE + [os.path.join(REPO, "tests", "node", "run_batch.mjs"), erased, cj, oj, "exact"], capture_output=True, text=True,
                       env=dict(os.environ, SPICEY_HIP_LIB=libpath), timeout=600)
    assert r.returncode == 0, r.stderr
    out = json.load(open(oj))
    assert "error" not in out, out
    py = simulateTRANBatch([parseNetlist(t) for _, t in items], exact_order=True)
    for i, ((name, _), t, p) in enumerate(zip(items, out["slots"], py)):
        if p is None:
            assert t is None, i
            continue
        if isinstance(p, Exception):
            assert t == {"error": "Singular matrix (real)"}, (i, t)
            continue
        assert t["keysV"] == list(p["nodeVoltages"]) and t["keysI"] == list(p["elementCurrents"]) and t["times"] == p["times"], i
        for k in t["keysV"]:
            assert bits_equal(farr(t["V"][k]), p["nodeVoltages"][k]).all(), (i, k)
        for k in t["keysI"]:
            assert bits_equal(farr(t["I"][k]), p["elementCurrents"][k]).all(), (i, k)
        assert t["skipRisk"] == p["skipRisk"], i
        if name is not None:
            run = load_golden(name)["runs"][0]
            assert t["keysV"] == run["keysV"] and t["times"] == run["times"]
            for k in run["keysV"]:
                assert bits_equal(farr(t["V"][k]), farr(run["V"][k])).all(), (name, k)
            assert t["state"]["vdPrev"] == run["state"]["D_vdPrev"] and t["state"]["vPrev"] == run["state"]["C_vPrev"]
