"""Builds and opens the CPU harnesses of tests/*_host: one `make` at a time per harness directory, its output in the error."""
import ctypes as C
import fcntl
import os
import subprocess


def make(here: str, target: str = "") -> None:
    """`make -s -C here [target]` under the directory's build lock (pytest-xdist workers: one build at a time); a failing
    build raises with everything make and the compiler printed."""
    os.makedirs(os.path.join(here, "_build"), exist_ok=True)
    with open(os.path.join(here, "_build", ".lock"), "w") as lk:
        fcntl.flock(lk, fcntl.LOCK_EX)
        p = subprocess.run(["make", "-s", "-C", here] + ([target] if target else []), capture_output=True, text=True)
        if p.returncode != 0:
            raise RuntimeError(f"make {target} failed in {here}:\n{p.stdout}{p.stderr}")


def load(here: str, so_name: str) -> C.CDLL:
    """The harness `here`/_build/`so_name`, brought up to date first."""
    make(here, os.path.join("_build", so_name))
    return C.CDLL(os.path.join(here, "_build", so_name))
