"""Circuits of the operand-slot tests (CPU and GPU) that spicey_amd.synth does not have: ground as the FIRST terminal."""
from spicey_amd import abi
from spicey_amd.netlist import parseNetlist


def reversed_chain_netlist(n: int, both_grounds: bool = False, tran: str = ".tran 1e-6 7e-5") -> str:
    """A diode-clamped RC chain whose elements to ground name ground first (`D 0 n`, `C 0 n`, `R 0 n`), so that ground is
    terminal a of the packed pair and the diodes point the other way; the source swings to both sides so that they conduct.
    both_grounds: also one resistor and one capacitor between ground and ground."""
    L = [f"* reversed chain n={n}", ".model DM D(Is=1e-14 N=1)", "V1 n1 0 PULSE(-5 5 0 1e-6 1e-6 4e-6 1e-5)"]
    for k in range(1, n):
        L.append(f"R{k} n{k} n{k+1} {100.0 * (1 + 0.001 * (k % 17)):.6g}")
        L.append(f"D{k} 0 n{k+1} DM")
        L.append(f"C{k} 0 n{k+1} {1e-9 * (1 + 0.002 * (k % 11)):.6g}")
        if k % 3 == 0:
            L.append(f"RG{k} 0 n{k+1} {1e4 * (1 + 0.003 * (k % 7)):.6g}")
    if both_grounds:
        L += ["RZ 0 0 50", "CZ 0 0 1e-9"]
    L += [tran, ".end", ""]
    return "\n".join(L)


def reversed_chain(n: int, n_inst: int = 1, both_grounds: bool = False, tran: str = ".tran 1e-6 7e-5"):
    """(flat, dt, steps, src) of reversed_chain_netlist; instance g > 0 gets slightly different resistors."""
    ckt = parseNetlist(reversed_chain_netlist(n, both_grounds, tran))
    dt, steps = abi.computeEffectiveTimeStep(ckt.analyses["tran"]["dt"], ckt.analyses["tran"]["tstop"])
    flat = abi.flatten(ckt).replicate(n_inst)
    for g in range(1, n_inst):
        flat.R_val[g] *= 1.0 + 0.01 * g
    return flat, dt, steps, abi.source_table(ckt, dt, steps)


def dense_rows_netlist(n: int, tran: str = ".tran 1e-6 7e-5") -> str:
    """A diode-clamped RC chain in which every fourth stage also has an antiparallel diode pair and a capacitor ACROSS its
    resistor: the node behind it gets a right-hand-side row of four contributions with both signs (two capacitors, two
    diodes), the off-diagonal entries of the stage two conductances each; every eighth stage a third diode to ground, which
    puts three conductances on a diagonal (the list form of phase B, beside the resident descriptors)."""
    L = [f"* dense rows n={n}", ".model DM D(Is=1e-14 N=1)", "V1 n1 0 PULSE(-3 3 0 1e-6 1e-6 4e-6 1e-5)"]
    for k in range(1, n):
        L.append(f"R{k} n{k} n{k+1} {100.0 * (1 + 0.001 * (k % 17)):.6g}")
        L.append(f"C{k} n{k+1} 0 {1e-9 * (1 + 0.002 * (k % 11)):.6g}")
        if k % 4 == 0:
            L += [f"DA{k} n{k} n{k+1} DM", f"DB{k} n{k+1} n{k} DM", f"CB{k} n{k} n{k+1} {2e-10 * (1 + 0.01 * (k % 5)):.6g}"]
        if k % 8 == 0:
            L.append(f"DG{k} n{k+1} 0 DM")
    L += [tran, ".end", ""]
    return "\n".join(L)


def dense_rows(n: int, n_inst: int = 1, tran: str = ".tran 1e-6 7e-5"):
    """(flat, dt, steps, src) of dense_rows_netlist; instance g > 0 gets slightly different resistors."""
    ckt = parseNetlist(dense_rows_netlist(n, tran))
    dt, steps = abi.computeEffectiveTimeStep(ckt.analyses["tran"]["dt"], ckt.analyses["tran"]["tstop"])
    flat = abi.flatten(ckt).replicate(n_inst)
    for g in range(1, n_inst):
        flat.R_val[g] *= 1.0 + 0.01 * g
    return flat, dt, steps, abi.source_table(ckt, dt, steps)
