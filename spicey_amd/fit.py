"""optimizeTRAN() / optimizeTRANBatch(): size elements so that transient measurements meet goals.

measureSens answers which element drives a number; optimizeTRAN asks the inverse: which L, C and R give 30 mV ripple, 5 V average
and a rise time under 2 us.  The method is damped least squares (Levenberg-Marquardt) on the element GAINS — factors on the
circuit's own values — with a Jacobian from central differences: per problem 1 + 2 nA variants of one topology (the nominal and,
per variable, the circuit with that element at (1 + h) and (1 - h) times its current value) are the instances of ONE transient
run per iteration.  The design is written on the device, the measurement passes of measureTRAN reduce every instance's waveforms
to rows that stay on the device, the scalar programs of spicey_amd/tran_mc.py turn them into x [n_inst][n_scalar], and one
workgroup per problem forms the normal equations, solves the damped system and moves the gains (spicey_run_fit,
include/spicey_hip.h, spicey_amd/csrc/fit_exec.h); a row of 8 doubles per problem and iteration comes back.

    optimizeTRAN(ckt, {"ripple": stats("v(out)", t_from=8e-4), "tr": rise_time("v(out)")},
                 goals={"ripple.pp": at_most(0.03), "ripple.avg": target(5.0, scale=0.01), "tr.time": at_most(2e-6)},
                 vars={"L1": (10e-6, 100e-6), "C1": (1e-6, 47e-6)})

measures and the "name.field" scalars are measureMonteCarlo's.  A goal is target(v), at_most(v), at_least(v) or between(lo, hi),
each with scale= (the residual is (x - bound) / scale; the default scale is max(|bound|, 1e-300)).  The scale is the goal's
tolerance unit: the loop stops at a cost F = sum r^2 <= f_tol = 1e-6, every goal within 1e-3 of its scale, or at a relative
step of the gains <= x_tol.  A field with a square root
(rms, rms_a, rms_b) goes down as its square: name it "name.rms^2" and square the target.  vars maps an element name to its
(low, high) bounds as element VALUES; the host turns them into gains on the circuit's value.  starts: None runs from the circuit's
own values (which must lie inside the bounds), an int k adds k - 1 starts drawn uniformly in the log of the bounds by a seeded
numpy generator, a list of {name: value} dicts gives the starts; they run as further problems of the same handle, the best
converged one is returned and all are listed.  There is no line search and no constraint between variables.

The result: values {element: value}, circuit (a copy with the values set; the input is not mutated), scalars {name.field:
value} at that point, cost, converged, status (0 converged, 1 max_iter reached, 2 the first point could not be evaluated,
3 singular system, 4 a value that is not finite, 5 stalled), iterations, history (a list of dicts of the row), fit_ms, kernel_ms,
starts (the same keys per start, without circuit).

design_reference_fit / reduce_reference_fit are the two kernels in numpy, bit for bit; host_run_fit is spicey_run_fit's loop on
the host — one reduced run of the backend per iteration on the design_reference_fit values, the numpy scalars and the numpy
update — for a backend without run_fit (the oracle), and the baseline and cross-check of the device loop.
"""
from __future__ import annotations

import copy
import math
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import abi
from .measure import _Plan
from .netlist import ParsedCircuit
from .sens import _elements
from .simulate import SingularMatrixError
from .tran_mc import _ALLOWED, compile_plan, eval_reference_scalars

DEFAULT_REL_STEP = 1e-3
TINY = 1e-300


# ---- goals ----------------------------------------------------------------------------------------------------------------------
def _goal(kind: int, lo: float, hi: float, scale: Optional[float], bound: float) -> tuple:
    for v in (lo, hi):
        if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v):
            raise ValueError(f"optimizeTRAN: a goal's bound must be a finite number, got {v!r}")
    if scale is None:
        scale = max(abs(bound), TINY)
    if isinstance(scale, bool) or not isinstance(scale, (int, float)) or not math.isfinite(scale) or not scale > 0:
        raise ValueError(f"optimizeTRAN: a goal's scale must be a finite number > 0, got {scale!r}")
    return ("goal", kind, float(lo), float(hi), 1.0 / float(scale))


def target(value: float, scale: Optional[float] = None) -> tuple:
    """x == value."""
    return _goal(abi.FIT_EQ, value, value, scale, value)


def at_most(value: float, scale: Optional[float] = None) -> tuple:
    """x <= value."""
    return _goal(abi.FIT_AT_MOST, 0.0, value, scale, value)


def at_least(value: float, scale: Optional[float] = None) -> tuple:
    """x >= value."""
    return _goal(abi.FIT_AT_LEAST, value, 0.0, scale, value)


def between(lo: float, hi: float, scale: Optional[float] = None) -> tuple:
    """lo <= x <= hi."""
    if not lo <= hi:
        raise ValueError(f"optimizeTRAN: between(lo, hi) needs lo <= hi, got {lo!r}, {hi!r}")
    return _goal(abi.FIT_BETWEEN, lo, hi, scale, max(abs(lo), abs(hi)))


# ---- the numpy restatements -----------------------------------------------------------------------------------------------------
def state_doubles(nA: int) -> int:
    """Doubles of one circuit's state between updates: A [nA][nA] | b [nA] | g_good [nA] | F_good | lambda | n_frozen."""
    return nA * nA + 2 * nA + 3


def design_reference_fit(R, Cv, Lv, act, step, g) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """The definition of spicey_fit_design_device in numpy: R (ohms), Cv, Lv [n_ckt W][n<kind>], act [nA], step [nA], g [n_ckt][nA]
    -> (R', C', L') of the same shapes: one product for the gain of a perturbed element, one for the value."""
    g = np.asarray(g, dtype=np.float64)
    n_ckt, nA = g.shape
    W = 1 + 2 * nA
    ni = n_ckt * W
    R, Cv, Lv = (np.asarray(a, dtype=np.float64).reshape(ni, -1) for a in (R, Cv, Lv))
    nR, nC = R.shape[1], Cv.shape[1]
    v = np.concatenate([R, Cv, Lv], axis=1)
    act = np.asarray(act, dtype=np.int64).reshape(-1)
    h = np.asarray(step, dtype=np.float64).reshape(-1)
    gain = np.repeat(g, W, axis=0).reshape(n_ckt, W, nA).copy()
    a = np.arange(nA)
    gain[:, 1 + 2 * a, a] = g * (1.0 + h)[None, :]
    gain[:, 2 + 2 * a, a] = g * (1.0 - h)[None, :]
    out = v.copy()
    out[:, act] = v[:, act] * gain.reshape(ni, nA)
    return out[:, :nR], out[:, nR:nR + nC], out[:, nR + nC:]


def _residuals(G, x0):
    """(r [n_scalar], active [n_scalar]) of goals G (abi.FIT_GOAL_DTYPE) at the nominal scalars x0 (no NaN)."""
    kind, lo, hi, w = G["kind"], G["lo"], G["hi"], G["weight"]
    with np.errstate(all="ignore"):
        eq = kind == abi.FIT_EQ
        above = ~eq & (kind != abi.FIT_AT_LEAST) & (x0 > hi)
        below = ~eq & ~above & (kind != abi.FIT_AT_MOST) & (x0 < lo)
        r = np.where(eq | below, w * (x0 - lo), np.where(above, w * (x0 - hi), 0.0))
    return r, eq | (r != 0.0)


def _update_one(req, first, h, lo, hi, G, ok, X, g, S):
    """One circuit's update: (g', row, done, S')."""
    nA = len(g)
    S = S.copy()
    A, b, gg, tail = S[:nA * nA].reshape(nA, nA), S[nA * nA:nA * nA + nA], S[nA * nA + nA:nA * nA + 2 * nA], S[nA * nA + 2 * nA:]
    x0 = X[0]
    F = np.inf
    r = active = None
    if ok[0] and not np.isnan(x0).any():
        r, active = _residuals(G, x0)
        F = 0.0
        with np.errstate(all="ignore"):
            for v in r:
                F = F + v * v
        if F != F:
            F = np.inf
    accepted = bool(np.isfinite(F)) if first else bool(F < tail[0])
    status, solve, maxd, n_clamped = 1, True, 0.0, 0
    if accepted:
        lam = req.lambda0 if first else tail[1] * req.lam_down
        with np.errstate(all="ignore"):
            J = G["weight"][:, None] * ((X[1::2] - X[2::2]).T / (2.0 * h)[None, :])  # [n_scalar][nA]
        J = J[active]
        frz = ~(ok[1::2] & ok[2::2]) | np.isnan(J).any(axis=0)
        A[:], b[:] = 0.0, 0.0
        with np.errstate(all="ignore"):
            for Jj, rj in zip(J, r[active]):
                A += Jj[:, None] * Jj[None, :]
                b += Jj * rj
        b[:] = -b
        A[frz, :], A[:, frz], b[frz] = 0.0, 0.0, 0.0
        gg[:] = g
        n_frozen = int(frz.sum())
        tail[0], tail[2] = F, n_frozen
        if F <= req.f_tol:
            status, solve = 0, False
    elif first:
        return g, np.array([F, np.inf, req.lambda0, 0.0, 2.0, 0.0, 0.0, 0.0]), 2, S
    else:
        lam = tail[1] * req.lam_up
        n_frozen = int(tail[2])
        if not lam <= req.lam_max:
            status, solve = 5, False
    d = None
    if solve:
        with np.errstate(all="ignore"):
            M = np.empty((nA, nA + 1))
            M[:, :nA], M[:, nA] = A, b
            dg = np.diagonal(A)
            M[np.arange(nA), np.arange(nA)] = np.where(dg == 0.0, 1.0, dg + lam * dg)
            for k in range(nA):
                col = np.abs(M[k:, k])
                col = np.where(np.isnan(col), -1.0, col)
                p = k + int(np.argmax(col))
                v = float(col[p - k])
                if v < 0.0:
                    p, v = k, 0.0
                if not v >= req.pivot_min:
                    status = 3
                    break
                if p != k:
                    M[[k, p], k:] = M[[p, k], k:]
                M[k + 1:, k] = M[k + 1:, k] / M[k, k]
                prod = M[k + 1:, k][:, None] * M[k, k + 1:][None, :]
                M[k + 1:, k + 1:] = M[k + 1:, k + 1:] - prod
            if status == 1:
                d = np.zeros(nA)
                for k in range(nA - 1, -1, -1):
                    d[k] = M[k, nA] / M[k, k]
                    prod = M[:k, k] * d[k]
                    M[:k, nA] = M[:k, nA] - prod
                if not np.isfinite(d).all():
                    status = 4
                else:
                    d = np.clip(d, -req.max_step, req.max_step)
                    maxd = float(np.abs(d).max())
                    if accepted and maxd <= req.x_tol:
                        status = 0
    if status == 1:
        v = gg * (1.0 + d)
        n_clamped = int(np.count_nonzero((v < lo) | (v > hi)))
        g = np.minimum(np.maximum(v, lo), hi)
    else:
        g = gg.copy()
    tail[1] = lam
    row = np.array([F, tail[0], lam, float(accepted), float(status), maxd, float(n_frozen), float(n_clamped)])
    return g, row, 0 if status == 1 else 1 if status == 0 else status, S


def reduce_reference_fit(req: abi.SpiceyFitReq, first: bool, step, g_lo, g_hi, goals, valid, x, g, done, state=None, rows=None):
    """(g', rows', done', state') of the update kernel: step [nA], g_lo / g_hi / g [n_ckt][nA], goals [n_ckt][n_scalar]
    (abi.FIT_GOAL_DTYPE), valid [n_ckt W] (None: all), x [n_ckt W][n_scalar], done [n_ckt], state [n_ckt][state_doubles(nA)] as the
    last update left it (None: zeros).  rows: what the array held before (a circuit that is done keeps it)."""
    g = np.array(g, dtype=np.float64)
    n_ckt, nA = g.shape
    W = 1 + 2 * nA
    x = np.asarray(x, dtype=np.float64).reshape(n_ckt, W, -1)
    ns = x.shape[2]
    G = np.ascontiguousarray(goals, dtype=abi.FIT_GOAL_DTYPE).reshape(n_ckt, ns)
    ok = np.ones((n_ckt, W), bool) if valid is None else np.asarray(valid).astype(bool).reshape(n_ckt, W)
    h = np.asarray(step, dtype=np.float64).reshape(nA)
    lo, hi = (np.asarray(a, dtype=np.float64).reshape(n_ckt, nA) for a in (g_lo, g_hi))
    done = np.array(done, dtype=np.int32)
    state = np.zeros((n_ckt, state_doubles(nA))) if state is None else np.array(state, dtype=np.float64).reshape(n_ckt, state_doubles(nA))
    rows = np.zeros((n_ckt, abi.FIT_ROW)) if rows is None else np.array(rows, dtype=np.float64)
    for c in range(n_ckt):
        if done[c]:
            continue
        g[c], rows[c], done[c], state[c] = _update_one(req, bool(first), h, lo[c], hi[c], G[c], ok[c], x[c], g[c].copy(), state[c])
    return g, rows, done, state


# ---- the loop on the host -------------------------------------------------------------------------------------------------------
def _with_values(flat: abi.FlatCircuit, R, Cv, Lv) -> abi.FlatCircuit:
    """`flat` with its instances' R, C and L values replaced."""
    kw = {k: getattr(flat, k) for k in abi.FlatCircuit.TOPO + abi.FlatCircuit.VALS}
    kw["R_val"], kw["C_val"], kw["L_val"] = R, Cv, Lv
    kw["S_ison"], kw["out_nodes"] = flat.S_ison, flat.out_nodes
    return abi.FlatCircuit(flat.n_nodes, flat.n_inst, **kw)


def host_run_fit(be, flat: abi.FlatCircuit, steps: int, dt: float, src: np.ndarray, req: abi.SpiceyFitReq, act, step, g_lo, g_hi, g0, goals, scalars, plan: _Plan) -> dict:
    """spicey_run_fit's loop on the host for any backend: per iteration the numpy design, ONE reduced run of the backend on a
    circuit that holds the designed values (plan.run: the backend's run_measure* or its run and the numpy reductions), the numpy
    scalars and the numpy update, until every circuit is done or max_iter is reached.  The result's keys are Handle.run_fit's."""
    n_ckt, nA, max_iter = int(req.n_ckt), int(req.nA), int(req.max_iter)
    W = 1 + 2 * nA
    if flat.n_inst != n_ckt * W:
        raise ValueError(f"fit: the handle has {flat.n_inst} instances, n_ckt W = {n_ckt * W} are needed (W = 1 + 2 nA = {W})")
    g = np.array(g0, dtype=np.float64).reshape(n_ckt, nA)
    ns = len(scalars)
    done, n_iter = np.zeros(n_ckt, np.int32), np.zeros(n_ckt, np.int32)
    state, rows = None, np.zeros((n_ckt, abi.FIT_ROW))
    history = np.zeros((max_iter, n_ckt, abi.FIT_ROW))
    F, xb = np.full(n_ckt, np.inf), np.full((n_ckt, ns), np.nan)
    out = {"status": abi.OK, "detail": "", "fit_ms": None, "tran_ms": None}
    ist = None
    for it in range(max_iter):
        res = plan.run(be, _with_values(flat, *design_reference_fit(flat.R_val, flat.C_val, flat.L_val, act, step, g)), steps, dt, src)
        if res["status"] not in (abi.OK, abi.ERR_SINGULAR):
            raise RuntimeError(res.get("detail") or f"spicey native error {res['status']}")
        ist = res.get("inst_status")
        if ist is None:
            if res["status"] != abi.OK:
                raise SingularMatrixError(res.get("detail", ""))
            ist = np.zeros(flat.n_inst, np.int32)
        elif res["status"] != abi.OK and not out["detail"]:
            out["detail"] = res.get("detail", "")
        valid = None if (np.asarray(ist) == 0).all() else (np.asarray(ist) == 0)
        x = eval_reference_scalars(scalars, tuple(res.get(k) for k in ("meas", "timing", "power")), valid)
        was = done.copy()
        g, rows, done, state = reduce_reference_fit(req, it == 0, step, g_lo, g_hi, goals, valid, x, g, done, state, rows)
        history[it] = rows
        for c in np.nonzero(was == 0)[0]:
            n_iter[c] += 1
            if rows[c, 4] != 2.0:
                F[c] = rows[c, 1]
            if rows[c, 3] == 1.0:
                xb[c] = x[c * W]
        if done.all():
            break
    status = np.where(done == 0, abi.FIT_MAX_ITER, np.where(done == 1, 0, done)).astype(np.int32)
    best = np.array(g0, dtype=np.float64).reshape(n_ckt, nA)
    if state is not None:
        best = np.where((status == abi.FIT_NOT_EVALUABLE)[:, None], best, state[:, nA * nA + nA:nA * nA + 2 * nA])
    out.update(g=best, F=F, x=xb, history=history[:int(n_iter.max())], n_iter=n_iter, ckt_status=status, inst_status=ist)
    return out


# ---- the API ------------------------------------------------------------------------------------------------------------------------
def _resolve_vars(ckt: ParsedCircuit, vars) -> Tuple[list, np.ndarray, np.ndarray, np.ndarray]:
    """(elements, act [nA] int32 ascending, lo [nA], hi [nA]: the bounds as gains on the circuit's values)."""
    elements = _elements(ckt)
    if not vars:
        raise ValueError("optimizeTRAN: no variables given (vars={element: (low, high)})")
    index = {n.upper(): e for e, (n, _, _) in enumerate(elements)}
    found = {}
    for key, pair in vars.items():
        e = index.get(str(key).upper())
        if e is None:
            raise ValueError(f"optimizeTRAN: vars names {key!r}, which is no R, C or L of the circuit")
        if not isinstance(pair, (tuple, list)) or len(pair) != 2 or any(isinstance(v, bool) or not isinstance(v, (int, float)) for v in pair):
            raise ValueError(f"optimizeTRAN: the bounds of {key!r} are (low, high) element values, got {pair!r}")
        lo, hi = float(pair[0]), float(pair[1])
        if not (math.isfinite(lo) and math.isfinite(hi) and 0.0 < lo <= hi):
            raise ValueError(f"optimizeTRAN: the bounds of {key!r} must be finite with 0 < low <= high, got {pair!r}")
        if e in found:
            raise ValueError(f"optimizeTRAN: vars names {key!r} twice")
        v = elements[e][2]
        if not v > 0.0:
            raise ValueError(f"optimizeTRAN: {key!r} has the value {v!r}; a gain needs a value > 0")
        found[e] = (lo / v, hi / v)
    act = np.array(sorted(found), dtype=np.int32)
    if len(act) > abi.FIT_MAX_NA:
        raise ValueError(f"optimizeTRAN: {len(act)} variables exceed the {abi.FIT_MAX_NA} of the update")
    return elements, act, np.array([found[int(e)][0] for e in act]), np.array([found[int(e)][1] for e in act])


def _resolve_goals(goals, names: List[str], root: np.ndarray) -> Tuple[List[str], np.ndarray, np.ndarray]:
    """(the goals' keys, idx [n_goal] into the compiled scalars, records [n_goal] of abi.FIT_GOAL_DTYPE)."""
    if not goals:
        raise ValueError("optimizeTRAN: no goals given")
    keys, idx, rows = [], [], []
    for key, spec in goals.items():
        if not (isinstance(spec, tuple) and len(spec) == 5 and spec[0] == "goal"):
            raise ValueError(f"optimizeTRAN: the goal of {key!r} is target(...), at_most(...), at_least(...) or between(...), got {spec!r}")
        name = key[:-2] if key.endswith("^2") else key
        if name not in names:
            raise ValueError(f"optimizeTRAN: goals names {key!r}, which no measure defines ({', '.join(names)})")
        j = names.index(name)
        if bool(root[j]) != key.endswith("^2"):
            if root[j]:
                raise ValueError(f"optimizeTRAN: {key!r} is a root field; the device carries its square: name it {key + '^2'!r} and square the target")
            raise ValueError(f"optimizeTRAN: {key!r}: only a root field (rms, rms_a, rms_b) has a square")
        keys.append(key)
        idx.append(j)
        rows.append(spec[1:])
    return keys, np.array(idx), abi.fit_goals(rows)


def _starts(starts, seed: int, elements, act, lo, hi) -> np.ndarray:
    """g0 [n_start][nA]."""
    nA = len(act)
    names = [elements[int(e)][0] for e in act]
    if starts is None or isinstance(starts, int) and not isinstance(starts, bool):
        k = 1 if starts is None else starts
        if k < 1:
            raise ValueError(f"optimizeTRAN: starts must be >= 1, got {starts!r}")
        if ((lo > 1.0) | (hi < 1.0)).any():
            bad = names[int(np.argmax((lo > 1.0) | (hi < 1.0)))]
            raise ValueError(f"optimizeTRAN: the bounds of {bad!r} do not contain the circuit's own value, where the first start stands: give starts=[{{...}}]")
        rng = np.random.default_rng(seed)
        drawn = np.exp(rng.uniform(np.log(lo), np.log(hi), (k - 1, nA)))
        return np.concatenate([np.ones((1, nA)), np.minimum(np.maximum(drawn, lo), hi)])
    out = np.ones((len(starts), nA))
    if not len(starts):
        raise ValueError("optimizeTRAN: starts is empty")
    for s, d in enumerate(starts):
        for key, v in d.items():
            if str(key).upper() not in [n.upper() for n in names]:
                raise ValueError(f"optimizeTRAN: a start names {key!r}, which is no variable")
            a = [n.upper() for n in names].index(str(key).upper())
            out[s, a] = float(v) / elements[int(act[a])][2]
        if ((out[s] < lo) | (out[s] > hi)).any():
            raise ValueError(f"optimizeTRAN: start {s} lies outside the bounds")
    return out


def _set_values(ckt: ParsedCircuit, values: Dict[str, float]) -> ParsedCircuit:
    out = copy.deepcopy(ckt)
    for lst, attr in ((out.R, "R"), (out.C, "C"), (out.L, "L")):
        for e in lst:
            if e.name in values:
                setattr(e, attr, values[e.name])
    return out


def optimizeTRANBatch(ckts: Sequence[ParsedCircuit], measures: Dict[str, object], goals: Dict[str, tuple], vars: Dict[str, tuple], starts=None, seed: int = 0,
                      max_iter: int = 30, rel_step: float = DEFAULT_REL_STEP, lambda0: float = 1e-3, lam_up: float = 10.0, lam_down: float = 0.1,
                      lam_max: float = 1e8, max_step: float = 0.5, x_tol: float = 1e-6, f_tol: float = 1e-6, exact_order: bool = False, *, device: int = 0,
                      backend=None) -> List[Optional[dict]]:
    """optimizeTRAN for circuits of ONE topology, dt and step count: one problem per circuit and start, all of them the circuits
    of one handle.  Slot i is optimizeTRAN(ckts[i], ...)'s result; None without a .tran card."""
    if exact_order and backend is not None:
        raise ValueError("optimizeTRAN: pass either backend= or exact_order=True, not both")
    for name, spec in (measures or {}).items():
        if not isinstance(spec, _ALLOWED):
            raise TypeError(f"optimizeTRAN: measure {name!r}: {type(spec).__name__.lower()} is not reduced across instances (stats, cross, when, "
                            "delay, rise_time, fall_time, settle, power and efficiency are)")
    if isinstance(rel_step, bool) or not isinstance(rel_step, (int, float)) or not 0.0 < rel_step < 1.0:
        raise ValueError(f"optimizeTRAN: rel_step must be a number in (0, 1), got {rel_step!r}")
    live = [i for i, c in enumerate(ckts) if c.analyses.get("tran")]
    out: List[Optional[dict]] = [None] * len(ckts)
    if not live:
        return out
    flats, srcs, g0s, los, his, infos = [], [], [], [], [], []
    plan0 = names = scalars = root = keys = idx = grec = act0 = None
    run = None
    for i in live:
        ckt = ckts[i]
        tran = ckt.analyses["tran"]
        dt, steps = abi.computeEffectiveTimeStep(tran["dt"], tran["tstop"])
        plan = _Plan(ckt, measures, dt, steps)
        try:
            nm, sc, rt = compile_plan(plan, dt)
        except TypeError as e:
            raise TypeError(str(e).replace("measureMonteCarlo", "optimizeTRAN")) from None
        elements, act, lo, hi = _resolve_vars(ckt, vars)
        if plan0 is None:
            plan0, names, scalars, root, act0, run = plan, nm, sc, rt, act, (dt, steps)
            keys, idx, grec = _resolve_goals(goals, names, root)
        elif plan.key() != plan0.key() or (dt, steps) != run or not np.array_equal(act, act0):
            raise ValueError("optimizeTRANBatch: the circuits must share topology, measured columns, dt, step count and variables")
        g0 = _starts(starts, seed, elements, act, lo, hi)
        W = 1 + 2 * len(act)
        one = plan.flatten(ckt)
        for _ in range(len(g0)):
            flats.append(one.replicate(W))
            srcs.append(abi.source_table(ckt, dt, steps))
        g0s.append(g0)
        los.append(np.repeat(lo[None, :], len(g0), axis=0))
        his.append(np.repeat(hi[None, :], len(g0), axis=0))
        infos.append((i, elements, len(g0)))
    nA, W = len(act0), 1 + 2 * len(act0)
    g0, g_lo, g_hi = np.concatenate(g0s), np.concatenate(los), np.concatenate(his)
    n_ckt = len(g0)
    if n_ckt * W > abi.MC_MAX_INST:
        raise ValueError(f"optimizeTRAN: {n_ckt} problems of {W} instances need {n_ckt * W}, more than {abi.MC_MAX_INST}")
    flat = abi.stack_instances(flats)
    shared = all(np.array_equal(t.view(np.int64), srcs[0].view(np.int64)) for t in srcs[1:])
    src = srcs[0] if shared else np.repeat(np.stack(srcs), W, axis=0)
    dt, steps = run
    sc = np.ascontiguousarray(scalars[idx])
    G = np.tile(grec, n_ckt).reshape(n_ckt, len(grec))
    step = np.full(nA, float(rel_step))
    req = abi.fit_req(n_ckt, nA, max_iter, lambda0, lam_up, lam_down, lam_max, max_step, x_tol, f_tol)
    if backend is None:
        from .lib import HipBackend  # fails loudly if the extension is missing

        backend = HipBackend(device=device, interpreter=3 if exact_order else 0)
    if hasattr(backend, "run_fit"):
        res = backend.run_fit(flat, steps, dt, src, req, act0, step, g_lo, g_hi, g0, G, sc, plan0.reqs, plan0.treqs, plan0.preqs)
    else:
        res = host_run_fit(backend, flat, steps, dt, src, req, act0, step, g_lo, g_hi, g0, G, sc, plan0)
    if res["status"] != abi.OK:
        err = ValueError if res["status"] == abi.ERR_BAD_DESC else SingularMatrixError if res["status"] == abi.ERR_SINGULAR else RuntimeError
        raise err(res.get("detail") or f"spicey native error {res['status']}")
    c0 = 0
    for i, elements, k in infos:
        per = []
        for c in range(c0, c0 + k):
            n_it = int(res["n_iter"][c])
            values = {elements[int(e)][0]: float(np.float64(elements[int(e)][2]) * res["g"][c, a]) for a, e in enumerate(act0)}
            per.append({"values": values, "scalars": {key: (None if math.isnan(v) else float(v)) for key, v in zip(keys, res["x"][c])}, "cost": float(res["F"][c]),
                        "converged": int(res["ckt_status"][c]) == abi.FIT_CONVERGED, "status": int(res["ckt_status"][c]), "iterations": n_it,
                        "history": [dict(zip(abi.FIT_ROW_KEYS, (float(v) for v in res["history"][t][c]))) for t in range(n_it)]})
        c0 += k
        order = sorted(range(k), key=lambda s: (not per[s]["converged"], per[s]["cost"] if not math.isnan(per[s]["cost"]) else math.inf, s))
        best = dict(per[order[0]])
        best.update(circuit=_set_values(ckts[i], best["values"]), fit_ms=res.get("fit_ms"), kernel_ms=res.get("tran_ms"), starts=per, best_start=order[0])
        out[i] = best
    return out


def optimizeTRAN(ckt: ParsedCircuit, measures: Dict[str, object], goals: Dict[str, tuple], vars: Dict[str, tuple], starts=None, seed: int = 0, max_iter: int = 30,
                 rel_step: float = DEFAULT_REL_STEP, **kw) -> Optional[dict]:
    """Element values of `ckt` that bring its transient measurements to `goals` (module text).  None without a .tran card.  The
    input circuit is not mutated; result["circuit"] is a copy with the values set."""
    return optimizeTRANBatch([ckt], measures, goals, vars, starts, seed, max_iter, rel_step, **kw)[0]
