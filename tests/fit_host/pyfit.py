"""ctypes view of the CPU harness of the element sizing (tests/fit_host/harness.cpp): the design and the update of fit_exec.h,
plus the inputs the host and GPU tests share."""
import ctypes as C
import os

import numpy as np

import harness_build
from noise_host.pynoise import Refused, bits_equal  # noqa: F401  (the tests' names for them)
from spicey_amd import abi
from spicey_amd import fit

HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None

SENTINEL = -7.25
NA = (1, 2, 5, 64, 65, 128)
NSCALAR = (1, 3, 70)
NCKT = (1, 3)
H = 2.0 ** -10
EXACT = ("one_step", "max_step", "bound", "reject", "stall", "inactive", "becomes_active", "nan_column", "singular", "damped", "invalid_first", "done_beside", "f_tol",
         "x_tol")


def lib():
    global _LIB
    if _LIB is None:
        L = harness_build.load(HERE, "libspicey_fit_host.so")
        vp, i32, i64 = C.c_void_p, C.c_int32, C.c_int64
        L.spicey_fit_host_workspace_bytes.restype = i64
        L.spicey_fit_host_workspace_bytes.argtypes = [i32, i32, i32]
        L.spicey_fit_host_lds_bytes.restype = i64
        L.spicey_fit_host_lds_bytes.argtypes = [i32]
        L.spicey_fit_host_state_offset.restype = i64
        L.spicey_fit_host_state_offset.argtypes = [i32, i32, i32]
        L.spicey_fit_host_state_doubles.restype = i64
        L.spicey_fit_host_state_doubles.argtypes = [i32]
        L.spicey_fit_host_design.restype = i32
        L.spicey_fit_host_design.argtypes = [i32, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, i64, C.c_char_p, i32]
        L.spicey_fit_host_update.restype = i32
        L.spicey_fit_host_update.argtypes = [vp, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, i64, i32, C.c_char_p, i32]
        assert L.spicey_fit_host_req_bytes() == C.sizeof(abi.SpiceyFitReq) and L.spicey_fit_host_goal_bytes() == abi.FIT_GOAL_DTYPE.itemsize
        assert L.spicey_fit_host_state_doubles(5) == fit.state_doubles(5)
        _LIB = L
    return _LIB


def _ptr(a):
    return a.ctypes.data if a is not None and a.size else None


def _f(a):
    return None if a is None else np.ascontiguousarray(a, dtype=np.float64)


def workspace(n_ckt, nA, n_scalar):
    """A zeroed workspace of exactly the bytes needed."""
    return np.zeros(max(lib().spicey_fit_host_workspace_bytes(n_ckt, nA, n_scalar), 8), np.uint8)


def state_of(work, n_ckt, nA, n_scalar):
    """[n_ckt][state_doubles] of a HOST copy of a workspace."""
    off = lib().spicey_fit_host_state_offset(n_ckt, nA, n_scalar)
    n = n_ckt * fit.state_doubles(nA)
    return work[off:off + 8 * n].view(np.float64).reshape(n_ckt, -1).copy()


def design(kinds, R, Cv, Lv, req, act, step, g, work=None, have_work=True):
    """(R', C', L') of the harness.  A refusal raises Refused with the judge's text, after checking that the results kept their
    sentinel."""
    R, Cv, Lv, g, step = _f(R), _f(Cv), _f(Lv), _f(g), _f(step)
    act = None if act is None else np.ascontiguousarray(act, dtype=np.int32)
    outs = [np.full(a.shape, SENTINEL) for a in (R, Cv, Lv)]
    if work is None:
        work = workspace(int(req.n_ckt), int(req.nA), 1) if req is not None and 1 <= req.nA <= 128 and req.n_ckt >= 1 else np.zeros(8, np.uint8)
    err = C.create_string_buffer(256)
    rc = lib().spicey_fit_host_design(*kinds, _ptr(R), _ptr(Cv), _ptr(Lv), C.addressof(req) if req is not None else None, _ptr(act), _ptr(step), _ptr(g),
                                      *(_ptr(o) for o in outs), work.ctypes.data if have_work else None, work.size, err, 256)
    if rc != abi.OK:
        assert rc == abi.ERR_BAD_DESC and all((o == SENTINEL).all() for o in outs)
        raise Refused(err.value.decode())
    return tuple(outs)


def update(req, first, step, g_lo, g_hi, goals, valid, x, g, done, work=None, rows=None, threads=0, have_work=True, n_scalar=None):
    """(g', rows, done', state') of the harness; `work` carries the circuits' state from one call to the next (None: a fresh one);
    rows start as SENTINEL unless given.  A refusal raises Refused, after checking that nothing was written."""
    g = np.array(g, dtype=np.float64)
    n_ckt, nA = g.shape
    x = _f(x)
    ns = (x.shape[-1] if x is not None else 0) if n_scalar is None else n_scalar
    goals = None if goals is None else np.ascontiguousarray(goals, dtype=abi.FIT_GOAL_DTYPE)
    valid = None if valid is None else np.ascontiguousarray(valid, dtype=np.uint8)
    done = np.array(done, dtype=np.int32)
    rows = np.full((n_ckt, abi.FIT_ROW), SENTINEL) if rows is None else np.array(rows, dtype=np.float64)
    if work is None:
        work = workspace(n_ckt, nA, max(ns, 1)) if req is not None and 1 <= req.nA <= 128 and req.n_ckt >= 1 else np.zeros(8, np.uint8)
    g0, r0, d0 = g.copy(), rows.copy(), done.copy()
    err = C.create_string_buffer(256)
    with np.errstate(all="ignore"):
        rc = lib().spicey_fit_host_update(C.addressof(req) if req is not None else None, ns, int(first), _ptr(_f(step)), _ptr(_f(g_lo)), _ptr(_f(g_hi)), _ptr(goals),
                                          _ptr(valid), _ptr(x), _ptr(g), _ptr(rows), _ptr(done), work.ctypes.data if have_work else None, work.size, threads, err, 256)
    if rc != abi.OK:
        assert rc == abi.ERR_BAD_DESC and bits_equal(g, g0).all() and bits_equal(rows, r0).all() and (done == d0).all()
        raise Refused(err.value.decode())
    return g, rows, done, state_of(work, n_ckt, nA, ns)


def reference_update(req, first, step, g_lo, g_hi, goals, valid, x, g, done, state=None, rows=None):
    """The numpy restatement on the same inputs and sentinels."""
    n_ckt = np.asarray(g).shape[0]
    return fit.reduce_reference_fit(req, first, step, g_lo, g_hi, goals, valid, x, g, done, state, np.full((n_ckt, abi.FIT_ROW), SENTINEL) if rows is None else rows)


# ---- shared inputs ----------------------------------------------------------------------------------------------------------
def model_x(B, t, G, s=1.0):
    """x [W][n_scalar] of the linear model x = t + B (g - s) for the gains G [W][nA] of the instances."""
    return t[None, :] + (np.asarray(G) - s) @ B.T


def inst_gains(g, step):
    """[n_ckt W][nA]: the gains of every instance of the design."""
    g = np.asarray(g, dtype=np.float64)
    n_ckt, nA = g.shape
    W = 1 + 2 * nA
    out = np.repeat(g, W, axis=0).reshape(n_ckt, W, nA).copy()
    a = np.arange(nA)
    out[:, 1 + 2 * a, a] = g * (1.0 + step)[None, :]
    out[:, 2 + 2 * a, a] = g * (1.0 - step)[None, :]
    return out.reshape(n_ckt * W, nA)


def random_case(nA, n_scalar, n_ckt, seed):
    """A seeded problem per circuit: (req, step, g_lo, g_hi, goals, x, g, done) with x from a random linear model around g, goals of
    every kind — some one-sided goals met, some not — and a well-conditioned J^T J + lambda diag where n_scalar >= nA (else the
    damping alone keeps the system regular)."""
    rng = np.random.default_rng(seed)
    req = abi.fit_req(n_ckt, nA, lambda0=1e-2)
    step = rng.choice([1e-3, 2.0 ** -9, 5e-4], nA)
    g = rng.uniform(0.6, 1.6, (n_ckt, nA))
    g_lo, g_hi = np.full((n_ckt, nA), 0.25), np.full((n_ckt, nA), 1.75)
    goals = np.zeros((n_ckt, n_scalar), abi.FIT_GOAL_DTYPE)
    xs = []
    for c in range(n_ckt):
        B = rng.normal(0.0, 1.0, (n_scalar, nA))
        B[np.arange(min(n_scalar, nA)), np.arange(min(n_scalar, nA))] += 3.0
        t = rng.normal(0.0, 1.0, n_scalar)
        x = model_x(B, t, inst_gains(g[c:c + 1], step))
        xs.append(x)
        for j in range(n_scalar):
            kind = (abi.FIT_EQ, abi.FIT_AT_MOST, abi.FIT_AT_LEAST, abi.FIT_BETWEEN)[j % 4] if j else abi.FIT_EQ
            off = rng.normal(0.0, 0.5)
            goals[c, j] = (kind, 0, x[0, j] + off - (0.25 if kind == abi.FIT_BETWEEN else 0.0), x[0, j] + off + (0.25 if kind == abi.FIT_BETWEEN else 0.0),
                           10.0 ** rng.uniform(-1, 1))
    return req, step, g_lo, g_hi, goals, np.concatenate(xs), g, np.zeros(n_ckt, np.int32)


def _goal(kind, lo, hi, w=1.0):
    return (kind, float(lo), float(hi), float(w))


def exact_case(name):
    """A named small case in representable numbers: dict(req, step, g_lo, g_hi, goals, calls=[dict(first, x, valid)], g, done,
    expect=[per call: dict(status, g, ...)]) — the calls run one after the other on ONE workspace.

    The model behind them: nA = 2, step h = 2^-10, x_j = t_j + B_j . (g - s) with B = diag(2, 4) and s = [0.75, 1.25] unless stated.
    From g = [1, 1] with EQ goals at t and weight 1: the Jacobian with respect to the RELATIVE change of a gain is B diag(g) = B
    exactly (every difference (x+ - x-) / 2h is a small dyadic number), r = B (g - s) = [0.5, -1], F = 1.25, J^T J = diag(4, 16),
    b = -J^T r = [-1, 4], and with lambda = 0 delta = [-0.25, 0.25]: g (1 + delta) = s, the solution, in one step."""
    B = np.array([[2.0, 0.0], [0.0, 4.0]])
    t = np.array([1.0, 2.0])
    s = np.array([0.75, 1.25])
    g = np.array([[1.0, 1.0]])
    step = np.array([H, H])
    kw = dict(lambda0=0.0, x_tol=0.0, f_tol=0.0, max_step=0.5, lam_up=4.0, lam_down=0.5, lam_max=64.0)
    lo, hi = np.array([[0.25, 0.25]]), np.array([[4.0, 4.0]])
    goals = [_goal(abi.FIT_EQ, t[0], t[0]), _goal(abi.FIT_EQ, t[1], t[1])]
    done = [0]

    def xs(gains, B=B, t=t, s=s):
        return model_x(B, t, inst_gains(np.atleast_2d(gains), step), s)

    calls = [dict(first=True, x=xs(g[0]), valid=None)]
    expect = [dict(status=1, accepted=1, F=1.25, F_good=1.25, d=0.25, g=[[0.75, 1.25]], lam=0.0, n_clamped=0, n_frozen=0)]
    if name == "one_step":
        pass
    elif name == "max_step":
        kw["max_step"] = 0.125
        expect = [dict(status=1, accepted=1, d=0.125, g=[[0.875, 1.125]], n_clamped=0)]
    elif name == "bound":
        lo = np.array([[0.875, 0.25]])
        expect = [dict(status=1, accepted=1, d=0.25, g=[[0.875, 1.25]], n_clamped=1)]
    elif name in ("reject", "stall"):
        kw["lambda0"] = 1.0   # M = diag(8, 32): delta = [-1/8, 1/8]
        first = dict(status=1, accepted=1, d=0.125, g=[[0.875, 1.125]], lam=1.0)
        worse = xs([2.0, 0.5])  # r = [2.5, -3]: F = 15.25 > 1.25, whatever the trial was
        calls.append(dict(first=False, x=worse, valid=None))
        # lambda = 4: M = diag(20, 80), delta = [-1/20, 4/80] — from the SAVED A and b, g_good = [1, 1] kept
        second = dict(status=1, accepted=0, F=15.25, F_good=1.25, lam=4.0, g=[[1.0 + -1.0 / 20.0, 1.0 + 4.0 / 80.0]], g_good=[1.0, 1.0])
        expect = [first, second]
        if name == "stall":
            calls += [dict(first=False, x=worse, valid=None)] * 3   # lambda 16, 64, then 256 > lam_max = 64
            expect += [dict(status=1, accepted=0, lam=16.0), dict(status=1, accepted=0, lam=64.0), dict(status=5, accepted=0, lam=256.0, g=[[1.0, 1.0]], done=5)]
    elif name in ("inactive", "becomes_active"):
        # a third scalar x_2 = 3 + 8 (g_0 - 0.75) = 5 under AT_MOST 6: inactive, a zero row; under AT_MOST 4 it is exceeded by 1:
        # r_2 = 1, J_2 = [8, 0]: A_00 = 4 + 64 = 68, b_0 = -(2 * 0.5 + 8 * 1) = -9, delta_0 = -9 / 68
        B3, t3 = np.array([[2.0, 0.0], [0.0, 4.0], [8.0, 0.0]]), np.array([1.0, 2.0, 3.0])
        cap = 6.0 if name == "inactive" else 4.0
        goals = goals + [_goal(abi.FIT_AT_MOST, 0.0, cap)]
        calls = [dict(first=True, x=xs(g[0], B3, t3), valid=None)]
        if name == "inactive":
            expect = [dict(status=1, accepted=1, F=1.25, g=[[0.75, 1.25]])]
        else:
            expect = [dict(status=1, accepted=1, F=2.25, g=[[1.0 + -9.0 / 68.0, 1.25]])]
    elif name == "nan_column":
        x = xs(g[0])
        x[3, 0] = np.nan   # instance 1 + 2 * 1: element 1 at +h — its column alone is frozen, element 0 moves as before
        calls = [dict(first=True, x=x, valid=None)]
        expect = [dict(status=1, accepted=1, n_frozen=1, g=[[0.75, 1.0]], d=0.25)]
    elif name in ("singular", "damped"):
        # two identical columns, s = [0.75, 1]: r = [0.5, 1]; A = [[20, 20], [20, 20]], b = [-5, -5]
        Bs = np.array([[2.0, 2.0], [4.0, 4.0]])
        calls = [dict(first=True, x=xs(g[0], Bs, t, np.array([0.75, 1.0])), valid=None)]
        if name == "singular":
            expect = [dict(status=3, accepted=1, F=1.25, g=[[1.0, 1.0]], done=3)]
        else:
            kw["lambda0"] = 1.0   # M = [[40, 20], [20, 40]]: delta = [-1/12, -1/12]
            expect = [dict(status=1, accepted=1, lam=1.0, close_g=[[1.0 - 1.0 / 12.0, 1.0 - 1.0 / 12.0]])]
    elif name == "invalid_first":
        calls = [dict(first=True, x=xs(g[0]), valid=[0, 1, 1, 1, 1])]
        expect = [dict(status=2, accepted=0, g=[[1.0, 1.0]], done=2, F=np.inf)]
    elif name == "done_beside":
        g = np.array([[1.0, 1.0], [1.0, 1.0]])
        lo, hi = np.tile(lo, (2, 1)), np.tile(hi, (2, 1))
        goals = goals + goals
        done = [1, 0]
        calls = [dict(first=True, x=xs(g), valid=None)]
        expect = [dict(status=[SENTINEL, 1], g=[[1.0, 1.0], [0.75, 1.25]])]
    elif name == "f_tol":
        kw["f_tol"] = 2.0   # F = 1.25 <= 2: converged at once, nothing solved, g stays
        expect = [dict(status=0, accepted=1, F=1.25, d=0.0, g=[[1.0, 1.0]], done=1)]
    elif name == "x_tol":
        kw["x_tol"] = 0.25  # max|d| = 0.25 <= x_tol on an accepted point: converged, g = g_good
        expect = [dict(status=0, accepted=1, d=0.25, g=[[1.0, 1.0]], done=1)]
    else:
        raise KeyError(name)
    n_ckt = len(g)
    return dict(req=abi.fit_req(n_ckt, 2, **kw), step=step, g_lo=lo, g_hi=hi, goals=abi.fit_goals(goals).reshape(n_ckt, -1), calls=calls, g=g,
                done=np.array(done, np.int32), expect=expect)
