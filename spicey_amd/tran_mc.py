"""measureMonteCarlo(): the distribution of transient measurements under component tolerances.

n samples of the circuit, each with its R, C and L drawn around the nominal values, are the instances of ONE transient run.  The
values are drawn on the device (spicey_run_mc, include/spicey_hip.h), the run reads them there, the measurement passes of
measureTRAN reduce every sample's waveforms to rows that stay on the device, small programs turn the rows into scalars — one per
numeric field of every measure, "name.field" — and a reduction ACROSS the samples, an LDS sort per scalar, brings back per
scalar the order statistics for the requested quantiles, the sum and the sum of squares, the count of samples outside a limit,
and the worst samples; per sample the number of scalars it violates.

    measureMonteCarlo(ckt, {"ripple": stats("v(out)", t_from=8e-4), "tr": rise_time("v(out)")}, tol={"L": 0.05, "C": 0.10}, n=1024,
                      quantiles=(0.01, 0.5, 0.99), limits={"ripple.pp": (None, 0.05), "tr.time": (0, 2e-6)})

measures is measureTRAN's dict, restricted to stats, cross, when, delay, rise_time / fall_time, settle (its two levels: the
later of two optional times is no arithmetic on a row), power and efficiency; any other kind is refused by name.  tol, dist and
nsigma are simulateMonteCarlo's; mc_values(ckt, tol, seed, s) of spicey_amd/mc.py rebuilds sample s as element values.

A scalar's program (abi.MC_SCALAR_DTYPE) pushes row fields and constants and combines them with one rounded operation per
instruction, in the order derive(), derive_timing(), derive_power() and derive_efficiency() of spicey_amd/measure.py use, so
eval_reference_scalars() — numpy — gives their numbers bit for bit.  What they report as None ("not found", p_source == 0) is NaN
here, through GUARD or an IEEE division.  A NaN sorts behind +inf, leaves the quantiles, mean and std (n_nan counts them) and
violates every limit of its scalar, also one that is not given.  Fields with a square root (rms, rms_a, rms_b) go down as their
square, without the clamp at 0: the quantiles take max(., 0) and the root on the host, since a monotone map commutes with order
statistics; their mean and std are None and their limits are squared on the way down.  power's apparent and pf are not
provided: they need two roots, and pf, which has a sign, is not monotone in its square.

reduce_reference_tran_mc() is the reduction in numpy (view(np.uint64), np.sort, the lane sum of spicey_amd/mc.py).

The result dict:
    scalars                {"name.field": {quantiles {p: value}, mean, std, n_valid, n_nan, yield, worst_low, worst_high, nominal}}
    yield                  the fraction of valid samples that violate no scalar
    failing                [(sample, the first scalar it violates)], ascending sample index
    n, n_valid, n_singular, n_stopped
    x                      with full=True: [n][n_scalar], the scalars of every sample as the device computed them
"""
from __future__ import annotations

import math
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import abi
from .mc import _lane_sum, _resolve
from .measure import Cross, Delay, Efficiency, Power, Settle, Stats, Transition, When, _Plan  # noqa: F401
from .netlist import ParsedCircuit
from .simulate import SingularMatrixError

_SIGN = np.uint64(1 << 63)
NAN_KEY = np.uint64(0xFFFFFFFFFFFFFFFE)
PAD_KEY = np.uint64(0xFFFFFFFFFFFFFFFF)
_ALLOWED = (Stats, Cross, When, Delay, Transition, Settle, Power, Efficiency)


# ---- programs -------------------------------------------------------------------------------------------------------------------
def F(p: int, row: int, field: int) -> tuple:
    return (abi.MCOP_FIELD, p, row, field, 0.0)


def K(c: float) -> tuple:
    return (abi.MCOP_CONST, 0, 0, 0, float(c))


ADD, SUB, MUL, DIV, GUARD = ((op, 0, 0, 0, 0.0) for op in (abi.MCOP_ADD, abi.MCOP_SUB, abi.MCOP_MUL, abi.MCOP_DIV, abi.MCOP_GUARD))


def make_scalars(programs: Sequence[Sequence[tuple]], check: bool = True) -> np.ndarray:
    """Programs (lists of F(...), K(...), ADD, SUB, MUL, DIV, GUARD) as records of abi.MC_SCALAR_DTYPE."""
    out = np.zeros(len(programs), abi.MC_SCALAR_DTYPE)
    for j, prog in enumerate(programs):
        if check and not 1 <= len(prog) <= abi.MC_SCALAR_INS:
            raise ValueError(f"a scalar's program has 1 to {abi.MC_SCALAR_INS} instructions, got {len(prog)}")
        out[j]["n_ins"] = len(prog)
        for i, ins in enumerate(prog[:abi.MC_SCALAR_INS]):
            out[j]["ins"][i] = ins
    return out


def _integral(p: int, row: int, f_sum: int, f_first: int, f_last: int, dt: float) -> list:
    """dt * (sum - (first + last) / 2)"""
    return [F(p, row, f_sum), F(p, row, f_first), F(p, row, f_last), ADD, K(2.0), DIV, SUB, K(dt), MUL]


def _mean_square(p: int, row: int, f_sq: int, f_first: int, f_last: int, dt: float, span: float) -> list:
    """dt * (sq - (first first + last last) / 2) / span"""
    return [F(p, row, f_sq), F(p, row, f_first), F(p, row, f_first), MUL, F(p, row, f_last), F(p, row, f_last), MUL, ADD, K(2.0), DIV, SUB, K(dt), MUL, K(span), DIV]


def _stats_fields(row: int, n: int, dt: float) -> List[Tuple[str, list, bool]]:
    p = abi.MC_PASS_MEASURE
    out = [("min", [F(p, row, 0)], False), ("max", [F(p, row, 1)], False), ("pp", [F(p, row, 1), F(p, row, 0), SUB], False),
           ("t_min", [F(p, row, 2), K(dt), MUL], False), ("t_max", [F(p, row, 3), K(dt), MUL], False), ("first", [F(p, row, 6)], False),
           ("final", [F(p, row, 7)], False)]
    if n > 1:
        span = (n - 1) * dt
        integ = _integral(p, row, 4, 6, 7, dt)
        out += [("integ", integ, False), ("avg", integ + [K(span), DIV], False), ("rms", _mean_square(p, row, 5, 6, 7, dt, span), True)]
    else:
        out += [("integ", [K(0.0)], False), ("avg", [F(p, row, 6)], False), ("rms", [F(p, row, 6), F(p, row, 6), MUL], True)]
    return out


def _cross_fields(row: int) -> List[Tuple[str, list, bool]]:
    p = abi.MC_PASS_MEASURE
    found = [F(p, row, 0), K(1.0), SUB, GUARD]  # count > 0
    return [("count", [F(p, row, 0)], False), ("t_first", found + [F(p, row, 1)], False), ("t_last", found + [F(p, row, 2)], False),
            # count >= 2; t_last - t_first >= 0; 0 / (t_last - t_first) is NaN exactly when the two are equal: t_last > t_first
            ("freq", [F(p, row, 0), K(2.0), SUB, GUARD, F(p, row, 2), F(p, row, 1), SUB, GUARD, K(0.0), F(p, row, 2), F(p, row, 1), SUB, DIV, GUARD,
                      F(p, row, 0), K(1.0), SUB, F(p, row, 2), F(p, row, 1), SUB, DIV], False)]


def _timing_fields(spec, row: int) -> List[Tuple[str, list, bool]]:
    p = abi.MC_PASS_TIMING

    def t(r, o):  # the time at field o + 1 if the crossing at field o was found
        return [F(p, r, o), GUARD, F(p, r, o + 1)]

    if isinstance(spec, When):
        return [("t", t(row, 3), False), ("level", [F(p, row, 5)], False), ("count", [F(p, row, 7)], False)]
    if isinstance(spec, Settle):
        return [("level_lo", [F(p, row, 5)], False), ("level_hi", [F(p, row + 1, 5)], False)]
    d = [F(p, row, 0), GUARD, F(p, row, 3), GUARD, F(p, row, 4), F(p, row, 1), SUB]
    if isinstance(spec, Transition):
        return [("t_start", t(row, 0), False), ("t_end", t(row, 3), False), ("time", d, False), ("level_start", [F(p, row, 2)], False),
                ("level_end", [F(p, row, 5)], False)]
    return [("t_trig", t(row, 0), False), ("t_targ", t(row, 3), False), ("delay", d, False), ("level_trig", [F(p, row, 2)], False),
            ("level_targ", [F(p, row, 5)], False), ("count_trig", [F(p, row, 6)], False), ("count_targ", [F(p, row, 7)], False)]


def _power_avg(row: int, n: int, dt: float) -> list:
    p = abi.MC_PASS_POWER
    return _integral(p, row, 4, 5, 6, dt) + [K((n - 1) * dt), DIV] if n > 1 else [F(p, row, 5)]


def _power_fields(row: int, n: int, dt: float) -> List[Tuple[str, list, bool]]:
    p = abi.MC_PASS_POWER
    out = [("energy", _integral(p, row, 4, 5, 6, dt) if n > 1 else [K(0.0)], False), ("avg", _power_avg(row, n, dt), False), ("peak", [F(p, row, 1)], False),
           ("t_peak", [F(p, row, 3), K(dt), MUL], False), ("min", [F(p, row, 0)], False), ("t_min", [F(p, row, 2), K(dt), MUL], False),
           ("first", [F(p, row, 5)], False), ("final", [F(p, row, 6)], False)]
    if n > 1:
        span = (n - 1) * dt
        out += [("rms_a", _mean_square(p, row, 7, 9, 10, dt, span), True), ("rms_b", _mean_square(p, row, 8, 11, 12, dt, span), True)]
    else:
        out += [("rms_a", [F(p, row, 9), F(p, row, 9), MUL], True), ("rms_b", [F(p, row, 11), F(p, row, 11), MUL], True)]
    return out


def _efficiency_fields(row: int, n_load: int, n_source: int, dt: float) -> List[Tuple[str, list, bool]]:
    p_load = _power_avg(row, n_load, dt)
    p_source = _power_avg(row + 1, n_source, dt) + [K(-1.0), MUL]
    # (0 / p_source is NaN exactly when p_source == 0, else a zero of either sign, which passes the guard)
    return [("p_load", p_load, False), ("p_source", p_source, False), ("eff", [K(0.0)] + p_source + [DIV, GUARD] + p_load + p_source + [DIV], False)]


def compile_plan(plan: _Plan, dt: float) -> Tuple[List[str], np.ndarray, np.ndarray]:
    """(names ["measure.field"], programs [n_scalar] of abi.MC_SCALAR_DTYPE, root [n_scalar] bool: the scalar is the square of its
    field) of a resolved measure dict, in the dict's order."""
    names, progs, root = [], [], []
    for name, kind, k in plan.names:
        if kind == "meas":
            r = plan.reqs[k]
            n = int(r["step_to"]) - int(r["step_from"]) + 1
            fields = _stats_fields(k, n, dt) if int(r["kind"]) == abi.MEAS_STATS else _cross_fields(k)
        elif isinstance(kind, Power):
            r = plan.preqs[k]
            fields = _power_fields(k, int(r["step_to"]) - int(r["step_from"]) + 1, dt)
        elif isinstance(kind, Efficiency):
            n0, n1 = (int(r["step_to"]) - int(r["step_from"]) + 1 for r in plan.preqs[k:k + 2])
            fields = _efficiency_fields(k, n0, n1, dt)
        elif isinstance(kind, (When, Delay, Transition, Settle)):
            fields = _timing_fields(kind, k)
        else:
            raise TypeError(f"measureMonteCarlo: measure {name!r}: {kind if isinstance(kind, str) else type(kind).__name__} is not reduced across samples")
        for field, prog, is_root in fields:
            names.append(f"{name}.{field}")
            progs.append(prog)
            root.append(is_root)
    return names, make_scalars(progs), np.asarray(root, dtype=bool)


# ---- the definitions in numpy ---------------------------------------------------------------------------------------------------
def eval_reference_scalars(scalars, rows: Sequence[Optional[np.ndarray]], valid=None) -> np.ndarray:
    """The definition of the scalar kernel in numpy: programs (abi.MC_SCALAR_DTYPE) over rows = (measure, timing, power), each
    [n_inst][n_rows][stride] or None -> x [n_inst][n_scalar]; one rounded operation per instruction, a NaN as np.nan's bits."""
    sc = np.ascontiguousarray(scalars, dtype=abi.MC_SCALAR_DTYPE).reshape(-1)
    ni = next(np.asarray(r).shape[0] for r in rows if r is not None and np.asarray(r).size)
    ok = np.ones(ni, bool) if valid is None else np.asarray(valid).astype(bool).reshape(ni)
    x = np.empty((ni, len(sc)))
    with np.errstate(all="ignore"):
        for j, P in enumerate(sc):
            st, bad = [], np.zeros(ni, bool)
            for I in P["ins"][:int(P["n_ins"])]:
                op = int(I["op"])
                if op == abi.MCOP_FIELD:
                    st.append(np.asarray(rows[int(I["pass"])], dtype=np.float64)[:, int(I["row"]), int(I["field"])].copy())
                elif op == abi.MCOP_CONST:
                    st.append(np.full(ni, float(I["c"])))
                elif op == abi.MCOP_GUARD:
                    bad |= ~(st.pop() >= 0.0)
                else:
                    b, a = st.pop(), st.pop()
                    st.append(a + b if op == abi.MCOP_ADD else a - b if op == abi.MCOP_SUB else a * b if op == abi.MCOP_MUL else a / b)
            v = st[0]
            x[:, j] = np.where(bad | np.isnan(v) | ~ok, np.nan, v)
    return x


def sort_keys(x: np.ndarray) -> np.ndarray:
    """The unsigned keys that order doubles as -inf < ... < -0 < +0 < ... < +inf < NaN."""
    u = np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)
    k = np.where((u & _SIGN) != 0, ~u, u | _SIGN)
    return np.where(np.isnan(x), NAN_KEY, k)


def unsort_keys(k: np.ndarray) -> np.ndarray:
    k = np.ascontiguousarray(k, dtype=np.uint64)
    u = np.where((k & _SIGN) != 0, k & ~_SIGN, ~k)
    return np.where(k >= NAN_KEY, np.nan, u.view(np.float64))


def reduce_reference_tran_mc(x, valid=None, lo=None, hi=None, probs=()) -> Tuple[np.ndarray, np.ndarray]:
    """The definition of the reduction in numpy: x [n_inst][n_scalar] -> (sample [n_inst][2] int64, stat [n_scalar][8 + 2 n_prob])."""
    x = np.asarray(x, dtype=np.float64)
    ni, ns = x.shape
    ok = np.ones(ni, bool) if valid is None else np.asarray(valid).astype(bool).reshape(ni)
    lo_ = np.full(ns, -np.inf) if lo is None else np.asarray(lo, dtype=np.float64)
    hi_ = np.full(ns, np.inf) if hi is None else np.asarray(hi, dtype=np.float64)
    probs = [float(p) for p in probs]
    with np.errstate(all="ignore"):
        viol = ~((x >= lo_[None, :]) & (x <= hi_[None, :]))
        sample = np.full((ni, 2), -1, np.int64)
        cnt = viol.sum(axis=1)
        first = np.where(cnt > 0, viol.argmax(axis=1), -1)
        sample[ok, 0], sample[ok, 1] = cnt[ok], first[ok]
        stat = np.zeros((ns, abi.TRAN_MC_STAT_HEAD + 2 * len(probs)))
        n_valid = int(ok.sum())
        keys = np.where(ok[:, None], sort_keys(x), PAD_KEY)
        for j in range(ns):
            srt = np.sort(keys[:, j])
            n_num = int(np.count_nonzero(srt < NAN_KEY))
            v = unsort_keys(srt[:n_num])
            stat[j, :5] = n_valid, n_num, np.count_nonzero(viol[ok, j]), _lane_sum(v[None, :])[0], _lane_sum((v * v)[None, :])[0]
            stat[j, 5] = int(np.argmax(keys[:, j] == srt[0])) if n_num else -1
            stat[j, 6] = int(np.argmax(keys[:, j] == srt[n_num - 1])) if n_num else -1
            for q, p in enumerate(probs):
                if n_num:
                    r = int(p * float(n_num - 1))
                    stat[j, 8 + 2 * q], stat[j, 9 + 2 * q] = v[r], v[min(r + 1, n_num - 1)]
                else:
                    stat[j, 8 + 2 * q] = stat[j, 9 + 2 * q] = np.nan
    return sample, stat


# ---- the public call ------------------------------------------------------------------------------------------------------------
def _limit_arrays(limits, names: List[str], root: np.ndarray) -> Tuple[Optional[np.ndarray], Optional[np.ndarray]]:
    if not limits:
        return None, None
    lo, hi = np.full(len(names), -np.inf), np.full(len(names), np.inf)
    for key, pair in limits.items():
        if key not in names:
            raise ValueError(f"measureMonteCarlo: limits names {key!r}, which is no scalar of these measures ({', '.join(names)})")
        if not isinstance(pair, (tuple, list)) or len(pair) != 2:
            raise ValueError(f"measureMonteCarlo: the limit of {key!r} is (low, high), either may be None, got {pair!r}")
        j = names.index(key)
        for side, v in enumerate(pair):
            if v is None:
                continue
            if isinstance(v, bool) or not isinstance(v, (int, float)) or math.isnan(v):
                raise ValueError(f"measureMonteCarlo: a limit of {key!r} is a number or None, got {v!r}")
            v = float(v)
            if root[j]:  # (the scalar is the field's square, the field itself is >= 0)
                v = (-np.inf if v <= 0 else v * v) if side == 0 else (-1.0 if v < 0 else v * v)
            (lo if side == 0 else hi)[j] = v
    return lo, hi


def _interp(a: float, b: float, p: float, n_num: int, is_root: bool) -> Optional[float]:
    if n_num == 0:
        return None
    pos = p * float(n_num - 1)
    v = a + (pos - math.floor(pos)) * (b - a)
    return math.sqrt(max(v, 0.0)) if is_root else v


def finish(x, root) -> np.ndarray:
    """The fields of scalars x [..., n_scalar]: max(., 0) and the root where the scalar is a square."""
    x = np.asarray(x, dtype=np.float64)
    with np.errstate(all="ignore"):
        return np.where(root, np.sqrt(np.where(np.isnan(x), np.nan, np.maximum(x, 0.0))), x)


def measureMonteCarlo(ckt: ParsedCircuit, measures: Dict[str, object], tol=None, n: int = 1024, seed: int = 0, dist="gauss", nsigma: float = 3,
                      quantiles: Sequence[float] = (0.01, 0.5, 0.99), limits: Optional[dict] = None, keep_first: bool = True, full: bool = False,
                      exact_order: bool = False, *, device: int = 0, backend=None) -> Optional[dict]:
    """Monte Carlo of the transient of `ckt`, measured by `measures` (module text).  None without a .tran card.  Raises
    SingularMatrixError when, with keep_first, the nominal circuit's run fails; a drawn sample whose run fails only leaves the
    statistics (n_singular).  backend: a test backend with run_tran_mc(flat, steps, dt, src, req, tol, icdf, scalars, lo, hi,
    probs, reqs, treqs, preqs, want_x)."""
    if tol is None:
        tol = {"R": 0.01, "C": 0.05}
    tran = ckt.analyses.get("tran")
    if not tran:
        return None
    if isinstance(n, bool) or not isinstance(n, int) or n < 1 or n > abi.MC_MAX_INST:
        raise ValueError(f"measureMonteCarlo: n must be an integer in [1, {abi.MC_MAX_INST}] (one workgroup sorts a scalar's samples), got {n!r}")
    if exact_order and backend is not None:
        raise ValueError("measureMonteCarlo: pass either backend= or exact_order=True, not both")
    for name, spec in (measures or {}).items():
        if not isinstance(spec, _ALLOWED):
            raise TypeError(f"measureMonteCarlo: measure {name!r}: {type(spec).__name__.lower()} is not reduced across samples (stats, cross, when, "
                            "delay, rise_time, fall_time, settle, power and efficiency are)")
    probs = [float(p) for p in quantiles]
    if any(not (0.0 <= p <= 1.0) for p in probs):
        raise ValueError("measureMonteCarlo: a quantile lies in [0, 1]")
    dt, steps = abi.computeEffectiveTimeStep(tran["dt"], tran["tstop"])
    plan = _Plan(ckt, measures, dt, steps)
    names, scalars, root = compile_plan(plan, dt)
    try:
        elements, t, icdf, log2K = _resolve(ckt, tol, dist, nsigma)
    except ValueError as e:
        raise ValueError(str(e).replace("simulateMonteCarlo", "measureMonteCarlo")) from None
    lo, hi = _limit_arrays(limits, names, root)
    if backend is None:
        from .lib import HipBackend  # fails loudly if the extension is missing

        backend = HipBackend(device=device, interpreter=3 if exact_order else 0)
    if not hasattr(backend, "run_tran_mc"):
        raise TypeError("measureMonteCarlo: the backend has no run_tran_mc")
    flat = plan.flatten(ckt).replicate(n)
    src = abi.source_table(ckt, dt, steps)
    req = abi.tran_mc_req(log2K, keep_first, seed)

    def run(be):
        res = be.run_tran_mc(flat, steps, dt, src, req, t, icdf, scalars, lo, hi, probs, plan.reqs, plan.treqs, plan.preqs, want_x=True)
        if res["status"] not in (abi.OK, abi.ERR_SINGULAR):
            raise RuntimeError(res.get("detail") or f"spicey native error {res['status']}")
        return res

    res = run(backend)
    if (np.asarray(res["inst_status"]) == -1).any() and hasattr(backend, "kw"):
        # (a sample stopped beside a singular one of its workgroup: once more, one sample per workgroup, the same draw)
        from .lib import HipBackend

        res = run(HipBackend(**{**backend.kw, "inst_per_wg": 1}))
    ist = np.asarray(res["inst_status"])
    if keep_first and int(ist[0]) != 0:
        raise SingularMatrixError(res.get("detail", ""))
    n_valid = int(np.count_nonzero(ist == 0))
    if n_valid == 0:  # (nothing was reduced: there is no statistic to report)
        raise SingularMatrixError(res.get("detail") or "measureMonteCarlo: no sample's run succeeded")
    stat, sample, x = res["stat"], res["sample"], res["x"]
    out = {}
    for j, name in enumerate(names):
        n_num, is_root = int(stat[j, 1]), bool(root[j])
        mean = std = None
        if n_num and not is_root:
            mean = float(stat[j, 3]) / n_num
            std = math.sqrt(max(float(stat[j, 4]) / n_num - mean * mean, 0.0))
        out[name] = {"quantiles": {p: _interp(float(stat[j, 8 + 2 * q]), float(stat[j, 9 + 2 * q]), p, n_num, is_root) for q, p in enumerate(probs)},
                     "mean": mean, "std": std, "n_valid": int(stat[j, 0]), "n_nan": int(stat[j, 0]) - n_num,
                     "yield": 1.0 - float(stat[j, 2]) / n_valid, "worst_low": int(stat[j, 5]) if n_num else None,
                     "worst_high": int(stat[j, 6]) if n_num else None,
                     "nominal": (None if math.isnan(x[0, j]) else float(finish(x[0, j], is_root))) if keep_first else None}
    bad = sample[:, 0] > 0
    result = {"scalars": out, "names": names, "yield": float(np.count_nonzero(sample[:, 0] == 0)) / n_valid,
              "failing": [(int(s), names[int(sample[s, 1])]) for s in np.nonzero(bad)[0]], "n": n, "n_valid": n_valid,
              "n_singular": int(np.count_nonzero(ist == abi.ERR_SINGULAR)), "n_stopped": int(np.count_nonzero(ist == -1)),
              "elements": [nm for nm, _, _ in elements], "tol": t.tolist(), "seed": int(seed), "mc_ms": res.get("mc_ms"), "draw_ms": res.get("draw_ms"),
              "kernel_ms": res.get("kernel_ms")}
    if full:
        result["x"] = finish(x, root[None, :])
    return result
