"""Records tests/golden/program_digest_parent.json: per case of tests/test_program_identity.py a digest of what
spicey_build_program hands to the rest of the library, plus a few counts of the program.

Run it with spicey_amd/csrc/symbolic.cpp at the content of the commit whose output is to be pinned (the parent of a
refactor), never with the code under test:  python tools/record_program_digest.py [--out FILE] [--times]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import test_program_identity as tpi  # noqa: E402


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=tpi.GOLDEN)
    ap.add_argument("--times", action="store_true", help="print the seconds each case took")
    a = ap.parse_args()
    out = {}
    for case in tpi.cases():
        for var in tpi.ENV_KNOBS:
            os.environ.pop(var, None)
        os.environ.update(case[4])
        t0 = time.perf_counter()
        out[case[0]] = tpi.record(case)
        if a.times:
            print(f"{time.perf_counter() - t0:7.3f} s  {case[0]}")
    for var in tpi.ENV_KNOBS:
        os.environ.pop(var, None)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"{len(out)} cases -> {a.out}")


if __name__ == "__main__":
    main()
