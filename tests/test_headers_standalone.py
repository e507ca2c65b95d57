"""Every piece of the transient phase code, its umbrella and the headers that include only the common piece compile on
their own: a translation unit that includes nothing but that header passes g++ -fsyntax-only (each includes what it uses)."""
import os
import subprocess

import pytest

from conftest import REPO

CSRC = os.path.join(REPO, "spicey_amd", "csrc")
# (tran_handle.h is not phase code: the host runtime's handle, which needs the HIP runtime's headers and is built with the library)
HOST_ONLY = ("tran_handle.h",)
HEADERS = sorted(f for f in os.listdir(CSRC) if f.startswith("tran_") and f.endswith(".h") and f not in HOST_ONLY) + ["fronts_exec.h", "ac_exec.h", "exact_exec.h"]


@pytest.mark.parametrize("header", HEADERS)
def test_header_compiles_alone(header, tmp_path):
    tu = tmp_path / "tu.cpp"
    tu.write_text(f'#include "{header}"\n')
    p = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-I", CSRC, str(tu)], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
