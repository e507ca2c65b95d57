"""Block-structured circuits whose dense fronts (spicey_amd/csrc/fronts_exec.h) have chosen shapes — test infrastructure.

A circuit is a tree of cliques: a separator clique, below it leaf cliques and, for a deeper tree, further separators with
leaves of their own.  Resistors join every pair of nodes inside a block and every node of a block to every node of the
separator above it; every leaf node has a capacitor to ground, every 7th leaf node a diode to ground (the circuit is
nonlinear: no factorisation is reused), and synth.PULSE drives one node of the root separator.  With front_cut = 1 the
nested dissection of the symbolic phase turns every block into one front whose boundary is the separator above it, so the
sizes of the blocks set (p, q) of every front — and with them which path of fronts_exec.h the front takes.  Which path
that is, is not restated here: tests/test_front_paths.py asks the engine's own predicates (emul.pyemul.front_census).

Values come from synth's LCG and are printed with repr, like every generator of spicey_amd/synth.py.
"""
from __future__ import annotations

from typing import List, Optional, Sequence, Union

import numpy as np

from spicey_amd import abi, synth
from spicey_amd.netlist import parseNetlist

# a leaf clique of that many nodes, or (separator size, [subtrees]), or (separator size, [subtrees], n): the same joined to
# the last n nodes of the separator above only
Tree = Union[int, tuple]

TRAN = ".tran 1e-6 6e-6"


def block_netlist(sep: int, leaves: Sequence[Tree], seed: int = 1, tran: str = TRAN, floating_pair: Optional[float] = None) -> str:
    """Netlist text of the tree (sep, leaves).  floating_pair = r: the last two nodes of the FIRST leaf clique (late pivots
    of its front) keep the ordinary resistor between them, every other resistor at either of them has r ohms, and they have
    no capacitor or diode — with r ~ 1e18 the pair floats as far as the arithmetic goes (conductances below the 1e-15
    pivot bound) while the circuit's structure, and with it every front, stays what it is for an ordinary r."""
    g = synth._LCG(seed)
    lines: List[str] = [f"* front blocks sep={sep} leaves={list(leaves)} seed={seed}", ".model DM D(Is=1e-14 N=1)"]
    count = {"R": 0, "C": 0, "D": 0, "blk": 0, "leafnode": 0}
    weak = set()
    if floating_pair is not None:
        assert isinstance(leaves[0], int)
        weak = {f"l1_{leaves[0] - 1}", f"l1_{leaves[0] - 2}"}  # (the root is block 0, the first leaf block 1)

    def res(a: str, b: str) -> None:
        count["R"] += 1
        r = 1000.0 * (1.0 + 0.1 * g.u())
        lines.append(f"R{count['R']} {a} {b} {synth._num(floating_pair if (a in weak) != (b in weak) else r)}")

    def clique(nodes: List[str]) -> None:
        for i, a in enumerate(nodes):
            for b in nodes[i + 1:]:
                res(a, b)

    def block(t: Tree, above: List[str]) -> List[str]:
        b = count["blk"]
        count["blk"] += 1
        if isinstance(t, tuple):
            nodes = [f"s{b}_{i}" for i in range(t[0])]
            clique(nodes)
            for a in nodes:
                for s in above[len(above) - t[2]:] if len(t) > 2 else above:
                    res(a, s)
            for sub in t[1]:
                block(sub, nodes)
            return nodes
        nodes = [f"l{b}_{i}" for i in range(t)]
        clique(nodes)
        for a in nodes:
            for s in above:
                res(a, s)
        for a in nodes:
            if a in weak:
                continue
            count["C"] += 1
            lines.append(f"C{count['C']} {a} 0 {synth._num(1e-9 * (1.0 + 0.1 * g.u()))}")
            if count["leafnode"] % 7 == 0:
                count["D"] += 1
                lines.append(f"D{count['D']} {a} 0 DM")
            count["leafnode"] += 1
        return nodes

    root = [f"s0_{i}" for i in range(sep)]
    count["blk"] = 1
    lines.append(f"V1 {root[0]} 0 {synth.PULSE}")
    clique(root)
    for sub in leaves:
        block(sub, root)
    lines += [tran, ".end", ""]
    return "\n".join(lines)


class Case:
    """One circuit of the family, parsed and flattened, with its run inputs."""

    def __init__(self, name: str, sep: int, leaves: Sequence[Tree], seed: int = 1, tran: str = TRAN, floating_pair: Optional[float] = None):
        self.name, self.sep, self.leaves, self.seed, self.tran, self.floating_pair = name, sep, list(leaves), seed, tran, floating_pair
        self.ckt = parseNetlist(block_netlist(sep, leaves, seed, tran, floating_pair))
        tr = self.ckt.analyses["tran"]
        self.dt, self.steps = abi.computeEffectiveTimeStep(tr["dt"], tr["tstop"])
        self.flat = abi.flatten(self.ckt)
        self.src = abi.source_table(self.ckt, self.dt, self.steps)

    def reseeded(self, seed: int, floating_pair: Optional[float] = None) -> "Case":
        return Case(self.name, self.sep, self.leaves, seed, self.tran, self.floating_pair if floating_pair is None else floating_pair)


def batch_of(cases: Sequence[Case]):
    """(flat, src[n_inst][steps + 1][nV]) of instances that share the topology of cases[0] and carry each case's values."""
    flat = cases[0].flat.replicate(len(cases))
    for i, c in enumerate(cases):
        for k in abi.FlatCircuit.TOPO:
            assert np.array_equal(getattr(c.flat, k), getattr(flat, k)), k
        for k in abi.FlatCircuit.VALS + ("S_ison",):
            getattr(flat, k)[i] = getattr(c.flat, k)[0]
    return flat, np.stack([c.src for c in cases])


# name: (separator, leaves).  What each case is FOR — the classes of fronts it holds — is asserted from the engine's own
# predicates in tests/test_front_paths.py::test_the_cases_hold_every_class_of_front.
SHAPES = {
    "two_even": (40, [70, 70]),
    "wide_boundary": (60, [90, 30]),
    "at_the_bound": (110, [105, 10]),
    "three_leaves": (50, [60, 40, 100]),
    "many_columns": (100, [30, 10]),
    # (the inner separator is joined to 20 of the root's 48 nodes only: joined to all of them its pivots would nest with the
    # root's and merge into the root front)
    "three_levels": (48, [(84, [40, 16], 20), 50]),
}
FRONT_CUT = 1
THREADS = 512  # what the full-size mesh runs with; the plan's own choice for circuits of this size is 256
# the singular case: a floating pair on the first leaf of the wide_boundary shape (a front staged by size, six panels)
FLOATING = ("wide_boundary", 1e18)
_CASES: dict = {}
_REFS: dict = {}
NCU = 256  # compute units of the MI355X (tests/test_launch_plan.py pins the plan on the same device)


def cpu_plan(flat: abi.FlatCircuit, **opts) -> dict:
    """SpiceyInfo of the launch plan spicey_create would make on an MI355X (the emulator library links the same spicey_plan)."""
    import ctypes as C

    from emul import pyemul
    d = flat.desc()
    o = abi.SpiceyOptions(**{k: int(v) for k, v in opts.items()})
    info = abi.SpiceyInfo()
    err = C.create_string_buffer(256)
    rc = pyemul.lib().spicey_emul_plan(C.byref(d), C.byref(o), NCU, 1, C.byref(info), err, len(err))
    assert rc == 0, err.value.decode()
    return info.as_dict()


def oracle_ref(c: "Case", oracle_backend) -> dict:
    """The oracle's run of the case, computed once per process and shared (callers do not modify it)."""
    key = (c.name, c.seed, c.floating_pair)
    if key not in _REFS:
        _REFS[key] = oracle_backend.run(c.flat, c.steps, c.dt, c.src)
    return _REFS[key]


def case(name: str) -> Case:
    """The case of that name, built once per process."""
    if name not in _CASES:
        sep, leaves = SHAPES[name]
        _CASES[name] = Case(name, sep, leaves, seed=11 + list(SHAPES).index(name))
    return _CASES[name]
