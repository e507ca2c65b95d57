"""measureSens() and measureWorstCase(): first-order sensitivities and tolerance corners of transient measurements.

The transient solver has no adjoint (DESIGN §26 is the AC engine's), so the method is SPICE's .sens / .wcase by finite
differences: 1 + 2 nA variants of one topology — the nominal circuit and, per toleranced element, the circuit with that element
at (1 + h) and (1 - h) times its value — are the instances of ONE transient run.  The design is written on the device
(spicey_run_sens, include/spicey_hip.h), the run reads it there, the measurement passes of measureTRAN reduce every instance's
waveforms to rows that stay on the device, the scalar programs of spicey_amd/tran_mc.py turn the rows into x [n_inst][n_scalar],
and a reduction ACROSS the instances brings back, per scalar "name.field" and active element,

    d = (x+ - x-) / (2 h)                  the change of the scalar per unit relative change of the element (dx / d ln v)
    c = ((x+ - x0) + (x- - x0)) / (h h)    the curvature

and per scalar the worst-case bound wc = sum |d| tol, rss2 = sum (d tol)^2, the dominant element and n_interior, the number of
elements with |d| < |c| tol: the parabola through the three points has its vertex inside the tolerance interval, so a corner need
not be the extreme.  measureWorstCase then runs the corners the signs of d point to — per scalar the vertex with every active
element at +sign tol (high) and -sign tol (low), identical vertices once — as the instances of a second run (spicey_run_levels).

    measureSens(ckt, {"ripple": stats("v(out)", t_from=8e-4)}, tol={"L": 0.05, "C": 0.10})
    measureWorstCase(ckt, {"ripple": stats("v(out)", t_from=8e-4)}, tol={"L": 0.05, "C": 0.10})

measures is measureMonteCarlo's dict (stats, cross, when, delay, rise_time / fall_time, settle, power, efficiency); tol is
resolved as simulateMonteCarlo's; the active elements are those with tol > 0.  rel_step, the h above, is a number or a per-kind /
per-name dict like tol (elements it does not name take 1e-3).  1e-3 is a documented default, not a tuned one: the truncation
error of d is O(h^2), its rounding error the scalars' relative error over 2 h.  Step-indexed fields (t_min, t_max, t_peak, count,
count_trig, ...) are piecewise constant in the element values: their differences are 0 or a jump of whole steps divided by 2 h,
not a derivative.

Fields with a square root (rms, rms_a, rms_b) go down as their square, as in measureMonteCarlo; the host applies the chain rule
d / (2 sqrt(x0)) to d, wc and rss (None where x0 <= 0); their curvature is None.

design_values() and reduce_reference_tran_sens() are the design and the reduction in numpy, bit for bit; design_circuit()
rebuilds one instance as element values.

The result of measureSens:
    scalars     {"name.field": {nominal, sens {element: d}, curvature {element: c} (None for a root field), wc, rss, linear_low,
                linear_high (nominal -+ wc), ranking (elements by |d| tol, descending, ties by index), dominant, n_interior, n_nan}}
                an entry is None where the scalar is NaN ("not found") or the element's perturbed run failed
    names, elements, active, tol, rel_step, n_singular, n_stopped, sens_ms, design_ms, kernel_ms
    x           with full=True: [1 + 2 nA][n_scalar], the fields of every instance as the device computed them
measureWorstCase adds per scalar corner_low, corner_high, corner_low_values, corner_high_values ({element: value}) and
monotone = (n_interior == 0), and n_corners, corner_ms, corner_kernel_ms, corner_levels (with full=True also corner_x).
"""
from __future__ import annotations

import math
from typing import Dict, List, Optional, Tuple

import numpy as np

from . import abi
from .mc import _lane_sum, _resolve
from .measure import _Plan
from .netlist import ParsedCircuit
from .sens import _elements
from .simulate import SingularMatrixError
from .tran_mc import _ALLOWED, compile_plan, finish

DEFAULT_REL_STEP = 1e-3


# ---- the definitions in numpy ---------------------------------------------------------------------------------------------------
def design_gains(n_inst: int, nE: int, act=None, step=None, lvl=None, tol=None) -> np.ndarray:
    """g [n_inst][nE], the factor of every element in every instance: ONE_AT_A_TIME from act [nA] and step [nA] (instance 1 + 2a
    has element act[a] at 1.0 + step[a], instance 2 + 2a at 1.0 - step[a]), or LEVELS from lvl [n_inst][nE] and tol [nE]
    (1.0 + lvl tol)."""
    if lvl is not None:
        lv = np.asarray(lvl, dtype=np.int8).reshape(n_inst, nE)
        return 1.0 + lv.astype(np.float64) * np.asarray(tol, dtype=np.float64).reshape(1, nE)
    act = np.asarray(act, dtype=np.int64).reshape(-1)
    step = np.asarray(step, dtype=np.float64).reshape(-1)
    if n_inst != 1 + 2 * len(act) or len(step) != len(act):
        raise ValueError("design_gains: n_inst = 1 + 2 nA, one step per active element")
    g = np.ones((n_inst, nE))
    a = np.arange(len(act))
    g[1 + 2 * a, act] = 1.0 + step
    g[2 + 2 * a, act] = 1.0 - step
    return g


def design_values(R, Cv, Lv, act=None, step=None, lvl=None, tol=None) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """The definition of spicey_tran_sens_design_device in numpy: nominal R (ohms), Cv, Lv [n_inst][n<kind>] -> (R', C', L') of the
    same shapes, the arrays the transient reads: one product each."""
    ni = np.asarray(R).shape[0]
    R, Cv, Lv = (np.asarray(a, dtype=np.float64).reshape(ni, -1) for a in (R, Cv, Lv))
    nR, nC, nL = R.shape[1], Cv.shape[1], Lv.shape[1]
    g = design_gains(ni, nR + nC + nL, act, step, lvl, tol)
    return R * g[:, :nR], Cv * g[:, nR:nR + nC], Lv * g[:, nR + nC:]


def reduce_reference_tran_sens(x, valid, step, tol_act) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """The definition of the reduction in numpy: x [1 + 2 nA][n_scalar], valid [n_inst] (or None), step [nA], tol_act [nA] ->
    (sens [n_scalar][nA][2], sign [n_scalar][nA] int8, bound [n_scalar][8])."""
    x = np.asarray(x, dtype=np.float64)
    ni, ns = x.shape
    h = np.asarray(step, dtype=np.float64).reshape(-1)
    t = np.asarray(tol_act, dtype=np.float64).reshape(-1)
    nA = len(h)
    if ni != 1 + 2 * nA or len(t) != nA:
        raise ValueError("reduce_reference_tran_sens: n_inst = 1 + 2 nA")
    ok = np.ones(ni, bool) if valid is None else np.asarray(valid).astype(bool).reshape(ni)
    sens = np.empty((ns, nA, 2))
    sign = np.zeros((ns, nA), np.int8)
    bound = np.zeros((ns, abi.TRAN_SENS_BOUND_ROW))
    with np.errstate(all="ignore"):
        for j in range(ns):
            x0, xp, xm = x[0, j], x[1::2, j], x[2::2, j]
            d = (xp - xm) / (2.0 * h)
            c = ((xp - x0) + (xm - x0)) / (h * h)
            num = ok[0] & ok[1::2] & ok[2::2] & ~np.isnan(x0) & ~np.isnan(xp) & ~np.isnan(xm) & ~np.isnan(d) & ~np.isnan(c)
            d, c = np.where(num, d, np.nan), np.where(num, c, np.nan)
            sens[j, :, 0], sens[j, :, 1] = d, c
            sign[j] = np.where(num, (d > 0).astype(np.int8) - (d < 0).astype(np.int8), 0)
            m = np.where(num, np.abs(d) * t, 0.0)  # (a lane adds from +0.0 and skips what is no number: + 0.0 changes no sum >= 0)
            dt = np.where(num, d * t, 0.0)
            n_num = int(num.sum())
            a_max = -1
            if n_num:
                top = np.max(np.where(num, np.abs(d) * t, -1.0))
                a_max = int(np.argmax(num & (np.abs(d) * t == top)))
            bound[j] = (x0 if ok[0] and not np.isnan(x0) else np.nan, _lane_sum(m[None, :])[0], _lane_sum((dt * dt)[None, :])[0], n_num, a_max,
                        np.abs(d[a_max]) * t[a_max] if n_num else 0.0, int(np.count_nonzero(num & (np.abs(d) < np.abs(c) * t))), 0.0)
    return sens, sign, bound


# ---- designs of a circuit -----------------------------------------------------------------------------------------------------
def _resolve_steps(elements, rel_step) -> np.ndarray:
    def one(v, what):
        if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v) or not 0.0 < v < 1.0:
            raise ValueError(f"measureSens: the relative step of {what} must be a finite number in (0, 1), got {v!r}")
        return float(v)

    if not isinstance(rel_step, dict):
        return np.full(len(elements), one(rel_step, "every element"))
    names = {n.upper() for n, _, _ in elements}
    by_name, by_kind = {}, {}
    for key, v in rel_step.items():
        k = str(key).upper()
        if k in names:
            by_name[k] = one(v, key)
        elif k in ("R", "C", "L"):
            by_kind[k] = one(v, f"kind {key}")
        else:
            raise ValueError(f"measureSens: rel_step names {key!r}, which is neither an R, C or L of the circuit nor a kind key")
    return np.array([by_name.get(n.upper(), by_kind.get(kind, DEFAULT_REL_STEP)) for n, kind, _ in elements], dtype=np.float64)


def _resolve_design(ckt: ParsedCircuit, tol, rel_step, who: str = "measureSens"):
    """(elements, tol [nE], act [nA] int32, step [nA]) of a circuit's one-at-a-time design."""
    try:
        elements, t, _, _ = _resolve(ckt, tol, "uniform", 1)
    except ValueError as e:
        raise ValueError(str(e).replace("simulateMonteCarlo", who).replace("tol * max|icdf| >= 1: a drawn value", "tol >= 1: a corner value")) from None
    act = np.nonzero(t > 0)[0].astype(np.int32)
    if not len(act):
        raise ValueError(f"{who}: no element has a tolerance > 0, so there is nothing to vary")
    return elements, t, act, _resolve_steps(elements, rel_step)[act]


def design_circuit(ckt: ParsedCircuit, tol, s: int, rel_step=DEFAULT_REL_STEP, levels=None) -> Dict[str, float]:
    """{element name: value} — ohms, farads, henries — of instance s of measureSens(ckt, tol=tol, rel_step=rel_step)'s design, or,
    with levels [n][nE] (int8 in {-1, 0, +1}, e.g. measureWorstCase's corner_levels), of row s of that LEVELS design.  Instance
    0 of the one-at-a-time design is nominal."""
    elements, t, act, h = _resolve_design(ckt, tol, rel_step)
    nE = len(elements)
    if levels is not None:
        lv = np.asarray(levels, dtype=np.int8).reshape(-1, nE)
        g = design_gains(1, nE, lvl=lv[s:s + 1], tol=t)[0]
    else:
        if not 0 <= s < 1 + 2 * len(act):
            raise ValueError(f"design_circuit: s in [0, {2 * len(act)}]")
        g = np.ones(nE)  # (row s of design_gains, without the other rows)
        if s > 0:
            a = (s - 1) // 2
            g[act[a]] = 1.0 - h[a] if (s - 1) % 2 else 1.0 + h[a]
    return {name: float(np.float64(value) * g[e]) for e, (name, _, value) in enumerate(elements)}


def corner_rows(sign, act, nE: int) -> Tuple[np.ndarray, np.ndarray]:
    """The level rows of the corners that sign [n_scalar][nA] points to: (lvl [n_rows][nE] int8, idx [n_scalar][2]) with row 0
    nominal, lvl[idx[j][0]] the high corner of scalar j (every active element at +sign) and lvl[idx[j][1]] its low corner (-sign);
    identical rows appear once, in the order they are first asked for."""
    sign = np.asarray(sign, dtype=np.int8)
    act = np.asarray(act, dtype=np.int64)
    rows, where = [np.zeros(nE, np.int8)], {np.zeros(nE, np.int8).tobytes(): 0}
    idx = np.zeros((sign.shape[0], 2), np.int64)
    for j in range(sign.shape[0]):
        for side, f in enumerate((1, -1)):
            row = np.zeros(nE, np.int8)
            row[act] = f * sign[j]
            k = where.setdefault(row.tobytes(), len(rows))
            if k == len(rows):
                rows.append(row)
            idx[j, side] = k
    return np.stack(rows), idx


# ---- the public calls -----------------------------------------------------------------------------------------------------------
def _num(v) -> Optional[float]:
    return None if math.isnan(v) else float(v)


class _Ctx:
    """What measureWorstCase takes over from the sensitivity run."""


def _run_with_repeat(backend, call):
    res = call(backend)
    if res["status"] not in (abi.OK, abi.ERR_SINGULAR):
        raise RuntimeError(res.get("detail") or f"spicey native error {res['status']}")
    if (np.asarray(res["inst_status"]) == -1).any() and hasattr(backend, "kw"):
        # (an instance stopped beside a singular one of its workgroup: once more, one instance per workgroup, the same design)
        from .lib import HipBackend

        res = call(HipBackend(**{**backend.kw, "inst_per_wg": 1}))
        if res["status"] not in (abi.OK, abi.ERR_SINGULAR):
            raise RuntimeError(res.get("detail") or f"spicey native error {res['status']}")
    return res


def _sens(who: str, ckt, measures, tol, rel_step, full, exact_order, device, backend):
    if tol is None:
        tol = {"R": 0.01, "C": 0.05}
    tran = ckt.analyses.get("tran")
    if not tran:
        return None, None
    if exact_order and backend is not None:
        raise ValueError(f"{who}: pass either backend= or exact_order=True, not both")
    for name, spec in (measures or {}).items():
        if not isinstance(spec, _ALLOWED):
            raise TypeError(f"{who}: measure {name!r}: {type(spec).__name__.lower()} is not reduced across instances (stats, cross, when, "
                            "delay, rise_time, fall_time, settle, power and efficiency are)")
    dt, steps = abi.computeEffectiveTimeStep(tran["dt"], tran["tstop"])
    plan = _Plan(ckt, measures, dt, steps)
    try:
        names, scalars, root = compile_plan(plan, dt)
    except TypeError as e:
        raise TypeError(str(e).replace("measureMonteCarlo", who)) from None
    elements, t, act, h = _resolve_design(ckt, tol, rel_step, who)
    nA = len(act)
    if 1 + 2 * nA > abi.MC_MAX_INST:
        raise ValueError(f"{who}: {nA} toleranced elements need {1 + 2 * nA} instances, more than {abi.MC_MAX_INST}")
    if backend is None:
        from .lib import HipBackend  # fails loudly if the extension is missing

        backend = HipBackend(device=device, interpreter=3 if exact_order else 0)
    if not hasattr(backend, "run_tran_sens") or not hasattr(backend, "run_tran_levels"):
        raise TypeError(f"{who}: the backend has no run_tran_sens / run_tran_levels")
    flat = plan.flatten(ckt).replicate(1 + 2 * nA)
    src = abi.source_table(ckt, dt, steps)
    req = abi.tran_sens_req(abi.TS_ONE_AT_A_TIME, nA)
    res = _run_with_repeat(backend, lambda be: be.run_tran_sens(flat, steps, dt, src, req, act, h, t, scalars, plan.reqs, plan.treqs, plan.preqs, want_x=True))
    ist = np.asarray(res["inst_status"])
    if int(ist[0]) != 0:
        raise SingularMatrixError(res.get("detail", ""))
    sens, sign, bound, x = res["sens"], res["sign"], res["bound"], res["x"]
    el_names = [elements[int(e)][0] for e in act]
    t_act = t[act]
    out = {}
    for j, name in enumerate(names):
        x0, is_root = float(bound[j, 0]), bool(root[j])
        # a root field went down as its square: the chain rule d sqrt(x) = dx / (2 sqrt(x0))
        k = 1.0
        if is_root:
            k = 1.0 / (2.0 * math.sqrt(x0)) if x0 > 0 else None
        d = [None if (math.isnan(v) or k is None) else float(v) * k for v in sens[j, :, 0]]
        nominal = None if math.isnan(x0) else float(finish(x0, is_root))
        wc = None if k is None else float(bound[j, 1]) * k
        rss = None if k is None else math.sqrt(float(bound[j, 2])) * k
        contrib = np.where(np.isnan(sens[j, :, 0]), -1.0, np.abs(sens[j, :, 0]) * t_act)
        order = [int(a) for a in np.argsort(-contrib, kind="stable") if contrib[a] >= 0]
        out[name] = {"nominal": nominal, "sens": dict(zip(el_names, d)),
                     "curvature": None if is_root else {nm: _num(v) for nm, v in zip(el_names, sens[j, :, 1])},
                     "wc": wc, "rss": rss, "linear_low": None if nominal is None or wc is None else nominal - wc,
                     "linear_high": None if nominal is None or wc is None else nominal + wc,
                     "ranking": [el_names[a] for a in order], "dominant": el_names[int(bound[j, 4])] if int(bound[j, 4]) >= 0 else None,
                     "n_interior": int(bound[j, 6]), "n_nan": nA - int(bound[j, 3])}
    result = {"scalars": out, "names": names, "elements": [nm for nm, _, _ in elements], "active": el_names, "tol": t.tolist(), "rel_step": h.tolist(),
              "n_singular": int(np.count_nonzero(ist == abi.ERR_SINGULAR)), "n_stopped": int(np.count_nonzero(ist == -1)), "sens_ms": res.get("sens_ms"),
              "design_ms": res.get("design_ms"), "kernel_ms": res.get("kernel_ms")}
    if full:
        result["x"] = finish(x, root[None, :])
    ctx = _Ctx()
    ctx.__dict__.update(plan=plan, names=names, scalars=scalars, root=root, elements=elements, t=t, act=act, sign=sign, backend=backend, dt=dt, steps=steps, src=src)
    return result, ctx


def measureSens(ckt: ParsedCircuit, measures: Dict[str, object], tol=None, rel_step=DEFAULT_REL_STEP, full: bool = False, exact_order: bool = False, *,
                device: int = 0, backend=None) -> Optional[dict]:
    """Sensitivities of the transient measurements `measures` of `ckt` to its toleranced R, C and L by central differences (module
    text).  None without a .tran card.  rel_step, default 1e-3, is not tuned; step-indexed fields (t_min, count, ...) are
    piecewise constant, so their differences are 0 or a jump.  Raises SingularMatrixError when the nominal circuit's run fails; a
    perturbed instance whose run fails makes that element's entries None (n_singular).  backend: a test backend with
    run_tran_sens(flat, steps, dt, src, req, act, step, tol, scalars, reqs, treqs, preqs, want_x) and run_tran_levels."""
    return _sens("measureSens", ckt, measures, tol, rel_step, full, exact_order, device, backend)[0]


def measureWorstCase(ckt: ParsedCircuit, measures: Dict[str, object], tol=None, rel_step=DEFAULT_REL_STEP, full: bool = False, exact_order: bool = False, *,
                     device: int = 0, backend=None) -> Optional[dict]:
    """measureSens, then the corners its signs point to as the instances of one more transient run (module text): per scalar
    corner_high / corner_low — the scalar at the vertex with every active element at +sign tol / -sign tol; an element whose
    sign is 0 stays nominal —, the element values there, and monotone = (n_interior == 0): only then is a corner the extreme to
    first and second order.  A corner whose run fails, or where the scalar is not found, is None."""
    result, c = _sens("measureWorstCase", ckt, measures, tol, rel_step, full, exact_order, device, backend)
    if result is None:
        return None
    nE = len(c.elements)
    lvl, idx = corner_rows(c.sign, c.act, nE)
    if len(lvl) > abi.MC_MAX_INST:
        raise ValueError(f"measureWorstCase: {len(lvl)} distinct corners, more than {abi.MC_MAX_INST} instances")
    flat = c.plan.flatten(ckt).replicate(len(lvl))
    req = abi.tran_sens_req(abi.TS_LEVELS, 0)
    res = _run_with_repeat(c.backend, lambda be: be.run_tran_levels(flat, c.steps, c.dt, c.src, req, lvl, c.t, c.scalars, c.plan.reqs, c.plan.treqs, c.plan.preqs))
    xc = finish(res["x"], c.root[None, :])
    g = design_gains(len(lvl), nE, lvl=lvl, tol=c.t)
    values = [{name: float(np.float64(value) * g[k, e]) for e, (name, _, value) in enumerate(c.elements)} for k in range(len(lvl))]
    for j, name in enumerate(c.names):
        s = result["scalars"][name]
        hi, lo = int(idx[j, 0]), int(idx[j, 1])
        s.update(corner_high=_num(xc[hi, j]), corner_low=_num(xc[lo, j]), corner_high_values=values[hi], corner_low_values=values[lo],
                 monotone=s["n_interior"] == 0)
    ist = np.asarray(res["inst_status"])
    result.update(n_corners=len(lvl) - 1, corner_levels=lvl, corner_index={name: (int(idx[j, 0]), int(idx[j, 1])) for j, name in enumerate(c.names)},
                  corner_ms=res.get("sens_ms"), corner_design_ms=res.get("design_ms"), corner_kernel_ms=res.get("kernel_ms"),
                  n_corner_singular=int(np.count_nonzero(ist == abi.ERR_SINGULAR)))
    if full:
        result["corner_x"] = xc
    return result
