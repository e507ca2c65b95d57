"""steadyState() / steadyStateBatch(): the periodic steady state of a driven circuit by shooting Newton.

Every analysis here starts a transient from the state the netlist carries — in practice the zero state.  Ripple, efficiency,
THD or yield of a converter are questions about the periodic steady state; steadyState finds the state s* that one period maps
onto itself by Newton on Phi(s) - s = 0, the Jacobian from finite differences of the state, and writes it into the circuit, so
the next simulateTRAN / measureTRAN / measureMonteCarlo starts there.

Definitions (include/spicey_hip.h, spicey_amd/csrc/pss_exec.h):
  period map   with m = period / dt (an integer), one period is a run of steps = m - 1: m solves on source rows 0 .. m - 1, each
               advancing the state by dt; Phi(s, on) is the state after it.  The steady state is the state ENTERING the solve at t = 0.
  state        x = [C_vprev | L_iprev | D_vdprev], nX entries; S_ison is carried, not differentiated.
  residual     res = max_a |Phi(s)_a - s_a| / (reltol max(|s_a|, |Phi(s)_a|) + abstol), vabstol for C and D entries, iabstol for L
               entries; converged: res <= 1 and the period returns the switch states it was entered with.
  instances    n_ckt W, W = 1 + nX (newton) or 1 (settle); instance c W + j belongs to circuit c, j = 0 nominal, j = 1 + a has
               entry a perturbed by rel_step max(|s_a|, 1 V or 1 mA).
One Newton iteration is ONE transient of all the instances over one period, the design before it and the dense update behind it on
the device (spicey_run_pss).  `damping` is a fixed factor; there is no line search.  nX <= 128 with Newton; method="settle"
(plain simulation, period by period, with the same stopping rule) takes any size.  A perturbation that moves a switching
instant across a time step makes the Jacobian noisy: a row's n_pert_switch_diff counts the perturbed instances whose end
switch states differ from the nominal's.

design_reference_pss / reduce_reference_pss are the numpy restatements of the design and the update, bit for bit; a backend
without run_pss (the oracle) is driven through them and its run().
"""
from __future__ import annotations

import math
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import abi
from .batch import write_state
from .netlist import ParsedCircuit
from .simulate import SingularMatrixError

PIVOT_MIN = 1e-12
STATE_KEYS = ("C_vprev", "L_iprev", "D_vdprev")


# ---- the numpy restatements ---------------------------------------------------------------------------------------------------
def _kind_arrays(kinds, v, i):
    """[nX] of `v` for the C and D entries and `i` for the L entries."""
    nC, nL, nD = kinds
    return np.concatenate([np.full(nC, v), np.full(nL, i), np.full(nD, v)])


def design_reference_pss(base, base_on, kinds, method: int = abi.PSS_NEWTON, rel_step: float = 1e-6, v_scale: float = 1.0, i_scale: float = 1e-3,
                         perturb: bool = True) -> Tuple[np.ndarray, np.ndarray, Optional[np.ndarray]]:
    """(X [n_ckt W][nX], on [n_ckt W][nS], h_eff [n_ckt][nX] or None) of the design kernel for base [n_ckt][nX], base_on [n_ckt][nS]
    and kinds = (nC, nL, nD)."""
    base = np.ascontiguousarray(base, dtype=np.float64)
    base_on = np.ascontiguousarray(base_on, dtype=np.int32).reshape(len(base), -1)
    n_ckt, nX = base.shape
    W = abi.pss_width(method, nX)
    X = np.repeat(base, W, axis=0).reshape(n_ckt, W, nX)
    h = None
    if perturb and method == abi.PSS_NEWTON:
        step = rel_step * np.maximum(np.abs(base), _kind_arrays(kinds, v_scale, i_scale)[None, :])
        sp = base + step
        h = sp - base
        a = np.arange(nX)
        X[:, 1 + a, a] = sp
    return X.reshape(n_ckt * W, nX), np.repeat(base_on, W, axis=0), h


def _update_one(b, bon, h, E, Eon, ist, method, damping, reltol, abst):
    """One circuit's update: (new base, new base_on, d or None, row, done)."""
    nX = len(b)
    W = len(E)
    e0 = E[0]
    row = np.zeros(abi.PSS_ROW)
    row[5] = -1.0
    with np.errstate(all="ignore"):
        fin = np.isfinite(b) & np.isfinite(e0)
        q = np.abs(e0 - b) / (reltol * np.maximum(np.abs(b), np.abs(e0)) + abst)
    q = np.where(fin, q, 0.0)
    if q.max() > 0.0:
        row[0], row[4] = q.max(), int(np.argmax(q))
    n_mis = int(np.count_nonzero(Eon[0] != bon))
    row[2] = n_mis
    row[6] = int(np.count_nonzero((Eon[1:] != Eon[0][None, :]).any(axis=1))) if W > 1 else 0
    ist = np.zeros(W, np.int32) if ist is None else np.asarray(ist)
    d = None
    if ist[0] > 0:
        status = 2
    elif ist[0] < 0:
        status = 5
    elif not fin.all():
        status = 4
    elif row[0] <= 1.0 and n_mis == 0:
        status = 0
    elif method == abi.PSS_SETTLE:
        status, d = 1, e0 - b
    elif (ist[1:] > 0).any():
        status = 4
    elif (ist[1:] < 0).any():
        status = 5
    else:
        status = 1
        with np.errstate(all="ignore"):
            M = np.empty((nX, nX + 1))
            M[:, :nX] = np.eye(nX) - ((E[1:] - e0[None, :]) / h[:, None]).T
            M[:, nX] = e0 - b
            if not np.isfinite(M).all():
                status = 4
            else:
                for k in range(nX):
                    col = np.abs(M[k:, k])
                    col = np.where(np.isnan(col), -1.0, col)
                    p = k + int(np.argmax(col))
                    v = float(col[p - k])
                    if v < 0.0:
                        p, v = k, 0.0
                    if row[5] < 0.0 or v < row[5]:
                        row[5] = v
                    if not v >= PIVOT_MIN:
                        status = 3
                        break
                    if p != k:
                        M[[k, p], k:] = M[[p, k], k:]
                    M[k + 1:, k] = M[k + 1:, k] / M[k, k]
                    prod = M[k + 1:, k][:, None] * M[k, k + 1:][None, :]
                    M[k + 1:, k + 1:] = M[k + 1:, k + 1:] - prod
                if status == 1:
                    d = np.zeros(nX)
                    for k in range(nX - 1, -1, -1):
                        d[k] = M[k, nX] / M[k, k]
                        prod = M[:k, k] * d[k]
                        M[:k, nX] = M[:k, nX] - prod
    if status == 1:
        with np.errstate(all="ignore"):
            if not np.isfinite(d).all():
                status, d = 4, None
            else:
                s = np.abs(d) / (reltol * np.abs(b) + abst)
                row[1] = s.max() if s.max() > 0.0 else 0.0
    row[3] = status
    row[7] = 1.0 if status == 0 else 0.0
    if status == 1:
        if method == abi.PSS_SETTLE:
            nb = e0.copy()
        else:
            move = damping * d
            nb = b + move
        return nb, Eon[0].copy(), d, row, 0
    return b, bon, None, row, 1 if status == 0 else status


def reduce_reference_pss(base, base_on, h_eff, end_x, end_on, done, kinds, method: int = abi.PSS_NEWTON, damping: float = 1.0, reltol: float = 1e-6,
                         vabstol: float = 1e-9, iabstol: float = 1e-12, ist=None, rows=None, delta=None):
    """(base', base_on', delta, rows, done') of the update kernel: base [n_ckt][nX], base_on [n_ckt][nS], h_eff [n_ckt][nX] (newton),
    the instances' END states end_x [n_ckt W][nX] and end_on [n_ckt W][nS], done [n_ckt], kinds = (nC, nL, nD), ist [n_ckt W] the
    instances' run statuses (None: all 0).  rows / delta: what the arrays held before (a circuit that is done, and the delta of one
    that did not move, keep it)."""
    base = np.array(base, dtype=np.float64)
    n_ckt, nX = base.shape
    base_on = np.array(base_on, dtype=np.int32).reshape(n_ckt, -1)
    W = abi.pss_width(method, nX)
    end_x = np.asarray(end_x, dtype=np.float64).reshape(n_ckt, W, nX)
    end_on = np.asarray(end_on, dtype=np.int32).reshape(n_ckt, W, -1)
    done = np.array(done, dtype=np.int32)
    rows = np.zeros((n_ckt, abi.PSS_ROW)) if rows is None else np.array(rows, dtype=np.float64)
    delta = np.zeros((n_ckt, nX)) if delta is None else np.array(delta, dtype=np.float64)
    abst = _kind_arrays(kinds, vabstol, iabstol)
    for c in range(n_ckt):
        if done[c]:
            continue
        i = None if ist is None else np.asarray(ist).reshape(n_ckt, W)[c]
        base[c], base_on[c], d, rows[c], done[c] = _update_one(base[c].copy(), base_on[c].copy(), None if h_eff is None else np.asarray(h_eff)[c], end_x[c], end_on[c],
                                                               i, method, damping, reltol, abst)
        if d is not None:
            delta[c] = d
    return base, base_on, delta, rows, done


def state_matrix(state: dict) -> np.ndarray:
    """[n_inst][nX] of a state dict's C_vprev | L_iprev | D_vdprev."""
    return np.concatenate([np.asarray(state[k], dtype=np.float64) for k in STATE_KEYS], axis=1)


def _with_state(flat: abi.FlatCircuit, X: np.ndarray, on: np.ndarray) -> abi.FlatCircuit:
    """`flat` with its instances' state replaced by the rows of X and on."""
    kw = {k: getattr(flat, k) for k in abi.FlatCircuit.TOPO + abi.FlatCircuit.VALS}
    kw["C_vprev"], kw["L_iprev"], kw["D_vdprev"] = X[:, :flat.nC], X[:, flat.nC:flat.nC + flat.nL], X[:, flat.nC + flat.nL:]
    kw["S_ison"], kw["out_nodes"] = on, flat.out_nodes
    return abi.FlatCircuit(flat.n_nodes, flat.n_inst, **kw)


def host_run_pss(be, flat: abi.FlatCircuit, m_steps: int, dt: float, src: np.ndarray, req: abi.SpiceyPssReq) -> dict:
    """spicey_run_pss's loop on the host for a backend that has run() only: the numpy design, one run of m_steps - 1 steps, the
    numpy update, until every circuit is done or max_iter is reached.  The result's keys are Handle.run_pss's."""
    kinds = (flat.nC, flat.nL, flat.nD)
    nX, n_ckt, method = sum(kinds), int(req.n_ckt), int(req.method)
    W = abi.pss_width(method, nX)
    if flat.n_inst != n_ckt * W:
        raise ValueError(f"pss: the handle has {flat.n_inst} instances, n_ckt W = {n_ckt * W} are needed")
    if method == abi.PSS_NEWTON and nX > abi.PSS_MAX_NX:
        raise ValueError(f'pss: nX = {nX} states exceed the {abi.PSS_MAX_NX} of the Newton update; method = "settle" takes any number')
    X0 = state_matrix({k: getattr(flat, k) for k in STATE_KEYS})
    base, base_on = X0[::W].copy(), flat.S_ison[::W].copy()
    done, n_iter = np.zeros(n_ckt, np.int32), np.zeros(n_ckt, np.int32)
    rows, delta = np.zeros((n_ckt, abi.PSS_ROW)), np.zeros((n_ckt, nX))
    history = np.zeros((int(req.max_iter), n_ckt, abi.PSS_ROW))
    out = {"status": abi.OK, "detail": ""}
    for it in range(int(req.max_iter)):
        X, on, h = design_reference_pss(base, base_on, kinds, method, req.rel_step, req.v_scale, req.i_scale)
        res = be.run(_with_state(flat, X, on), m_steps - 1, dt, src)
        if res["status"] not in (abi.OK, abi.ERR_SINGULAR):
            raise RuntimeError(res.get("detail") or f"spicey native error {res['status']}")
        ist = res.get("inst_status")
        if ist is None:
            if res["status"] != abi.OK:
                raise SingularMatrixError(res.get("detail", ""))
            ist = np.zeros(flat.n_inst, np.int32)
        elif res["status"] != abi.OK and not out["detail"]:
            out["detail"] = res.get("detail", "")
        n_iter += done == 0
        st = res["state"]
        base, base_on, delta, rows, done = reduce_reference_pss(base, base_on, h, state_matrix(st), st["S_ison"], done, kinds, method, req.damping, req.reltol,
                                                                req.vabstol, req.iabstol, ist, rows, delta)
        history[it] = rows
        if done.all():
            break
    out.update(x=base, on=base_on, history=history[:int(n_iter.max())], n_iter=n_iter, ckt_status=np.where(done == 0, abi.PSS_MAX_ITER, np.where(done == 1, 0, done)).astype(np.int32))
    return out


# ---- the period -------------------------------------------------------------------------------------------------------------------
def common_period(ckt: ParsedCircuit) -> float:
    """The common period of the circuit's PULSE sources: their equal `per`, or the largest when the others divide it."""
    pers = []
    for vs in ckt.V:
        spec = getattr(vs.waveform, "spec", None) if vs.waveform is not None else None
        if vs.waveform is None:
            continue
        if spec is None or spec[0] != "pulse":
            raise ValueError("steadyState: a source is not a PULSE (PWL or other waveform): pass period=")
        per = float(spec[1]["period"])
        if not (math.isfinite(per) and per > 0.0):
            raise ValueError("steadyState: a PULSE source has no positive period: pass period=")
        pers.append(per)
    if not pers:
        raise ValueError("steadyState: the circuit has no periodic source (DC only): pass period=")
    top = max(pers)
    for per in pers:
        k = top / per
        if abs(k - round(k)) > 1e-9 * k:
            raise ValueError("steadyState: the PULSE periods are incommensurate: pass period=")
    return top


def steps_per_period(period: float, dt: float) -> int:
    """m = period / dt, which must be an integer >= 1 (judged on |m - round(m)| <= 1e-9 m)."""
    if not (math.isfinite(period) and period > 0.0):
        raise ValueError("steadyState: period must be positive and finite")
    m = period / dt
    if round(m) < 1 or abs(m - round(m)) > 1e-9 * m:
        raise ValueError(f"steadyState: period = {period!r} is not a whole number of time steps dt = {dt!r} (period / dt = {m!r})")
    return int(round(m))


def period_table(ckt: ParsedCircuit, dt: float, m: int) -> np.ndarray:
    """The source rows 0 .. m - 1 of one period; row m must repeat row 0 within 1e-9 |v| + 1e-12."""
    tab = abi.source_table(ckt, dt, m)
    if (np.abs(tab[m] - tab[0]) > 1e-9 * np.abs(tab[0]) + 1e-12).any():
        raise ValueError("steadyState: the sources are not periodic in `period` (the source row at t = period differs from the row at t = 0)")
    return np.ascontiguousarray(tab[:m])


# ---- the API ------------------------------------------------------------------------------------------------------------------------
def _flatten_one_node(ckt: ParsedCircuit) -> abi.FlatCircuit:
    """One recorded node, no matter what the netlist prints: a steady-state run reads the end state only."""
    flat = abi.flatten(ckt)
    if flat.n_nodes >= 1:
        flat.out_nodes = np.array([1], np.int32)
    return flat


def _state_dict(ckt: ParsedCircuit, x: np.ndarray, on: np.ndarray) -> dict:
    nC, nL = len(ckt.C), len(ckt.L)
    D = [d for d in ckt.D if d.model is not None]
    S = [s for s in ckt.S if s.model is not None]
    return {"C": {e.name: float(x[k]) for k, e in enumerate(ckt.C)}, "L": {e.name: float(x[nC + k]) for k, e in enumerate(ckt.L)},
            "D": {e.name: float(x[nC + nL + k]) for k, e in enumerate(D)}, "S": {e.name: bool(on[k]) for k, e in enumerate(S)}}


def _result(ckt: ParsedCircuit, res: dict, c: int, W: int, period: float, m: int, method: str, write_back: bool) -> dict:
    status, n_iter = int(res["ckt_status"][c]), int(res["n_iter"][c])
    hist = [dict(zip(abi.PSS_ROW_KEYS, (float(v) for v in res["history"][k][c]))) for k in range(n_iter)]
    x, on = res["x"][c], res["on"][c]
    out = {"converged": status == abi.PSS_CONVERGED, "status": status, "iterations": n_iter, "periods_simulated": n_iter * W,
           "residual": hist[-1]["res"] if hist else math.nan, "history": hist, "period": period, "steps_per_period": m, "method": method,
           "state": _state_dict(ckt, x, on)}
    if out["converged"] and write_back:
        nC, nL = len(ckt.C), len(ckt.L)
        write_state(ckt, {"C_vprev": x[None, :nC], "L_iprev": x[None, nC:nC + nL], "D_vdprev": x[None, nC + nL:], "S_ison": on[None, :]}, 0)
    return out


def _run(be, flat: abi.FlatCircuit, m: int, dt: float, src: np.ndarray, req: abi.SpiceyPssReq) -> dict:
    res = be.run_pss(flat, m, dt, src, req) if hasattr(be, "run_pss") else host_run_pss(be, flat, m, dt, src, req)
    if res["status"] not in (abi.OK, abi.ERR_SINGULAR):
        err = ValueError if res["status"] == abi.ERR_BAD_DESC else RuntimeError
        raise err(res.get("detail") or f"spicey native error {res['status']}")
    return res


def steadyStateBatch(ckts: Sequence[ParsedCircuit], period: Optional[float] = None, method: str = "newton", max_iter: int = 20, damping: float = 1.0,
                     reltol: float = 1e-6, vabstol: float = 1e-9, iabstol: float = 1e-12, rel_step: float = 1e-6, write_back: bool = True, backend=None, *,
                     device: int = 0, max_instances: int = 4096) -> List[object]:
    """The periodic steady state of every circuit in `ckts`; circuits that share topology, dt and period are the circuits of ONE
    handle (n_ckt W instances).  Slot i is steadyState(ckts[i], ...)'s result, or — its nominal run singular — the
    SingularMatrixError, returned instead of raised; a circuit without .tran gives None.  A circuit stopped by another's failure
    in its workgroup runs again in a second call without the failed ones."""
    if method not in abi.PSS_METHODS:
        raise ValueError(f'steadyState: method must be "newton" or "settle", not {method!r}')
    if len({id(c) for c in ckts}) != len(ckts):
        raise ValueError("steadyStateBatch: the same circuit object appears twice (its state would be written twice)")
    meth = abi.PSS_METHODS[method]
    out: List[object] = [None] * len(ckts)
    groups: Dict[tuple, List[int]] = {}
    info = {}
    for i, c in enumerate(ckts):
        tran = c.analyses.get("tran")
        if not tran:
            continue
        dt, _ = abi.computeEffectiveTimeStep(tran["dt"], tran["tstop"])
        per = float(period) if period is not None else common_period(c)
        m = steps_per_period(per, dt)
        flat = _flatten_one_node(c)
        info[i] = (dt, per, m, flat, period_table(c, dt, m))
        topo = tuple(getattr(flat, k).tobytes() for k in abi.FlatCircuit.TOPO)
        groups.setdefault((flat.n_nodes, topo, dt, m), []).append(i)
    if backend is None and groups:
        from .lib import HipBackend  # fails loudly if the extension is missing

        backend = HipBackend(device=device)
    for idx in groups.values():
        dt, per, m, flat0, _ = info[idx[0]]
        nX = flat0.nC + flat0.nL + flat0.nD
        if nX == 0:
            raise ValueError("steadyState: the circuit has no state (no capacitor, inductor or diode)")
        if meth == abi.PSS_NEWTON and nX > abi.PSS_MAX_NX:
            raise ValueError(f'steadyState: nX = {nX} states exceed the {abi.PSS_MAX_NX} of the Newton update; method="settle" takes any number')
        W = abi.pss_width(meth, nX)
        per_launch = max(1, max_instances // W)
        for a in range(0, len(idx), per_launch):
            pending = idx[a:a + per_launch]
            while pending:
                flat = abi.stack_instances([info[i][3].replicate(W) for i in pending])
                tabs = [info[i][4] for i in pending]
                shared = all(np.array_equal(t.view(np.int64), tabs[0].view(np.int64)) for t in tabs[1:])
                src = tabs[0] if shared else np.repeat(np.stack(tabs), W, axis=0)
                req = abi.pss_req(len(pending), meth, max_iter, damping, reltol, vabstol, iabstol, rel_step)
                res = _run(backend, flat, m, dt, src, req)
                again = []
                for c, i in enumerate(pending):
                    s = int(res["ckt_status"][c])
                    if s == abi.PSS_NOMINAL_SINGULAR:
                        out[i] = SingularMatrixError(res.get("detail", ""))
                    elif s == abi.PSS_STOPPED:
                        again.append(i)
                    else:
                        out[i] = _result(ckts[i], res, c, W, per, m, method, write_back)
                if len(again) == len(pending):
                    raise RuntimeError("steadyStateBatch: a launch settled none of its circuits")
                pending = again
    return out


def steadyState(ckt: ParsedCircuit, period: Optional[float] = None, method: str = "newton", max_iter: int = 20, damping: float = 1.0, reltol: float = 1e-6,
                vabstol: float = 1e-9, iabstol: float = 1e-12, rel_step: float = 1e-6, write_back: bool = True, backend=None, *, device: int = 0) -> Optional[dict]:
    """The periodic steady state of `ckt` under its periodic sources.  period: None takes the common period of the PULSE sources.
    Returns {converged, status, iterations, periods_simulated, residual, history, period, steps_per_period, method, state: {"C":
    {name: v}, "L": {name: i}, "D": {name: vd}, "S": {name: bool}}}; status 0 converged, 1 max_iter reached, 3 singular Jacobian, 4 a
    value that is not finite.  Converged and write_back: the state goes into `ckt` (vPrev, iPrev, vdPrev, isOn) and the next
    simulateTRAN / measureTRAN starts in steady state; otherwise `ckt` is untouched and nothing is raised.  A singular nominal run
    raises what simulateTRAN raises.  None without a .tran card."""
    out = steadyStateBatch([ckt], period, method, max_iter, damping, reltol, vabstol, iabstol, rel_step, write_back, backend, device=device)[0]
    if isinstance(out, Exception):
        raise out
    return out
