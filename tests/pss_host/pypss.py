"""ctypes view of the CPU harness of the periodic steady state (tests/pss_host/harness.cpp): the design and the update of
pss_exec.h, plus the inputs the host and GPU tests share."""
import ctypes as C
import os

import numpy as np

import harness_build
from noise_host.pynoise import Refused, bits_equal  # noqa: F401  (the tests' names for them)
from spicey_amd import abi
from spicey_amd import pss

HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None

SENTINEL = -7.25
SENTINEL_I = -99
NX = (1, 2, 63, 64, 65, 128)
NCKT = (1, 3)
EXACT = ("row_exchange", "equal_pivots", "last_exchange", "singular", "nan_perturbed", "done_beside", "converged", "converged_switch_mismatch", "damping",
         "settle", "h_representable", "nominal_singular", "perturbed_singular", "stopped")


def lib():
    global _LIB
    if _LIB is None:
        L = harness_build.load(HERE, "libspicey_pss_host.so")
        vp, i32, i64 = C.c_void_p, C.c_int32, C.c_int64
        L.spicey_pss_host_workspace_bytes.restype = i64
        L.spicey_pss_host_workspace_bytes.argtypes = [i32, i32, i32]
        L.spicey_pss_host_lds_bytes.restype = i64
        L.spicey_pss_host_lds_bytes.argtypes = [i32, i32]
        L.spicey_pss_host_design.restype = i32
        L.spicey_pss_host_design.argtypes = [i32, i32, i32, i32, vp, i32, vp, vp, vp, vp, vp, vp, vp, i32, i64, C.c_char_p, i32]
        L.spicey_pss_host_update.restype = i32
        L.spicey_pss_host_update.argtypes = [i32, i32, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, i32, i64, i32, C.c_char_p, i32]
        assert L.spicey_pss_host_req_bytes() == C.sizeof(abi.SpiceyPssReq)
        _LIB = L
    return _LIB


def _ptr(a):
    return a.ctypes.data if a is not None and a.size else None


def split(X, kinds):
    """(Cv, Li, Dv) [n][n<kind>] contiguous, of X [n][nX]."""
    nC, nL, _ = kinds
    return tuple(np.ascontiguousarray(a) for a in (X[:, :nC], X[:, nC:nC + nL], X[:, nC + nL:]))


def kinds_of(nX):
    """(nC, nL, nD) with every kind present from nX = 3 on."""
    return ((nX + 2) // 3, (nX + 1) // 3, nX // 3)


def design(kinds, req, base, base_on, perturb=True, have_work=True, work_bytes=-1):
    """(X [n_inst][nX], on [n_inst][nS], h [n_ckt][nX]) of the harness.  A refusal raises Refused with the judge's text, after
    checking that the results kept their sentinel."""
    base = np.ascontiguousarray(base, dtype=np.float64)
    n_ckt = base.shape[0]
    base_on = np.ascontiguousarray(base_on, dtype=np.int32).reshape(n_ckt, -1)
    nX, nS = sum(kinds), base_on.shape[1]
    ni = max(n_ckt * abi.pss_width(int(req.method), nX), 1) if req is not None else n_ckt
    parts = [np.full((ni, k), SENTINEL) for k in kinds]
    on = np.full((ni, nS), SENTINEL_I, np.int32)
    h = np.full((n_ckt, max(nX, 1)), SENTINEL)
    err = C.create_string_buffer(256)
    rc = lib().spicey_pss_host_design(*kinds, nS, C.addressof(req) if req is not None else None, int(perturb), _ptr(base), _ptr(base_on), _ptr(h), *(_ptr(p) for p in parts),
                                      _ptr(on), int(have_work), work_bytes, err, 256)
    if rc != abi.OK:
        assert rc == abi.ERR_BAD_DESC and all((p == SENTINEL).all() for p in parts) and (on == SENTINEL_I).all() and (h == SENTINEL).all()
        raise Refused(err.value.decode())
    return np.concatenate(parts, axis=1), on, h


def update(kinds, req, base, base_on, h, X, on, done, ist=None, threads=0, have_work=True, work_bytes=-1):
    """(base', base_on', delta, rows, done') of the harness for the END states X [n_inst][nX] and on [n_inst][nS]; delta and rows
    start as SENTINEL.  threads: the emulated workgroup.  A refusal raises Refused, after checking that nothing was written."""
    base = np.array(base, dtype=np.float64)
    n_ckt = base.shape[0]
    base_on = np.array(base_on, dtype=np.int32).reshape(n_ckt, -1)
    nX, nS = sum(kinds), base_on.shape[1]
    parts = split(np.ascontiguousarray(X, dtype=np.float64).reshape(-1, max(nX, 1))[:, :nX], kinds)
    on = np.ascontiguousarray(on, dtype=np.int32)
    done = np.array(done, dtype=np.int32)
    h = None if h is None else np.ascontiguousarray(h, dtype=np.float64)
    ist = None if ist is None else np.ascontiguousarray(ist, dtype=np.int32)
    delta, rows = np.full((n_ckt, max(nX, 1)), SENTINEL), np.full((n_ckt, abi.PSS_ROW), SENTINEL)
    b0, on0, d0 = base.copy(), base_on.copy(), done.copy()
    err = C.create_string_buffer(256)
    with np.errstate(all="ignore"):
        rc = lib().spicey_pss_host_update(*kinds, nS, C.addressof(req) if req is not None else None, _ptr(ist), _ptr(base), _ptr(base_on), _ptr(h), *(_ptr(p) for p in parts),
                                          _ptr(on), _ptr(delta), _ptr(rows), _ptr(done), int(have_work), work_bytes, threads, err, 256)
    if rc != abi.OK:
        assert rc == abi.ERR_BAD_DESC and bits_equal(base, b0).all() and (base_on == on0).all() and (done == d0).all()
        assert (delta == SENTINEL).all() and (rows == SENTINEL).all()
        raise Refused(err.value.decode())
    return base, base_on, delta[:, :nX], rows, done


def reference_update(kinds, req, base, base_on, h, X, on, done, ist=None):
    """The numpy restatement on the same inputs and sentinels."""
    n_ckt, nX = np.asarray(base).shape
    return pss.reduce_reference_pss(base, base_on, h, X, on, done, kinds, int(req.method), req.damping, req.reltol, req.vabstol, req.iabstol, ist,
                                    np.full((n_ckt, abi.PSS_ROW), SENTINEL), np.full((n_ckt, nX), SENTINEL))


# ---- shared inputs ----------------------------------------------------------------------------------------------------------
def linear_case(nX, n_ckt, seed, nS=2):
    """A seeded affine period map per circuit: (kinds, req, base, base_on, h, X_end, on_end, done, J) with |J_ia| <= 0.9 / nX, so
    that M = I - J is strictly diagonally dominant and cond_inf(M) <= 19; the design is the numpy one."""
    rng = np.random.default_rng(seed)
    kinds = kinds_of(nX)
    req = abi.pss_req(n_ckt)
    base = rng.normal(0.0, 1.0, (n_ckt, nX)) * 10.0 ** rng.uniform(-3, 1, (n_ckt, nX))
    base_on = rng.integers(0, 2, (n_ckt, nS)).astype(np.int32)
    J = rng.uniform(-0.9 / nX, 0.9 / nX, (n_ckt, nX, nX))
    g = rng.normal(0.0, 1.0, (n_ckt, nX))
    X, on, h = pss.design_reference_pss(base, base_on, kinds, abi.PSS_NEWTON, req.rel_step, req.v_scale, req.i_scale)
    W = 1 + nX
    E = np.einsum("cia,cwa->cwi", J, X.reshape(n_ckt, W, nX)) + g[:, None, :]
    on_end = on.copy().reshape(n_ckt, W, nS)
    on_end[:, :, 0] ^= 1          # every instance leaves with another switch state than it entered with
    if nX > 1:
        on_end[:, 2, -1] ^= 1     # one perturbed instance ends apart from the nominal
    return kinds, req, base, base_on, h, E.reshape(n_ckt * W, nX), on_end.reshape(n_ckt * W, nS), np.zeros(n_ckt, np.int32), J


def fd_matrix(base, h, X):
    """(M [n_ckt][nX][nX], r [n_ckt][nX]) as the update forms them, in numpy."""
    n_ckt, nX = base.shape
    E = X.reshape(n_ckt, 1 + nX, nX)
    e0 = E[:, 0]
    M = np.eye(nX)[None] - np.transpose((E[:, 1:] - e0[:, None, :]) / h[:, :, None], (0, 2, 1))
    return M, e0 - base


H2 = 2.0 ** -10


def _dyadic(M, r, base, n_ckt=1):
    """END states of capacitor-only circuits whose finite differences are EXACTLY I - M's off-identity part: rel_step = 2^-10,
    |base| <= 1, so h = 2^-10, and every entry a small dyadic number."""
    M, r, base = np.asarray(M, float), np.asarray(r, float), np.asarray(base, float)
    nX = len(r)
    J = np.eye(nX) - M
    E = np.empty((1 + nX, nX))
    E[0] = base + r
    for a in range(nX):
        E[1 + a] = E[0] + J[:, a] * H2
    return E


def exact_case(name):
    """A named small case: dict(kinds, req, base, base_on, h, X, on, done, ist, expect) with expect = dict(status=[..], delta=...,
    base=...) of what is known exactly."""
    nS = 1
    kw = {}
    ist = None
    M = [[2.0, 1.0], [1.0, 2.0]]
    r = [0.5, -0.5]                                      # with the default M: d = [1/2, -1/2]
    base = [0.5, -0.25]
    expect = {}
    if name == "row_exchange":
        M, r = [[0.0, 1.0], [1.0, 1.0]], [0.5, 1.5]       # M[0][0] = 0: rows 0 and 1 change places at k = 0
        expect = {"status": [1], "delta": [[1.0, 0.5]], "min_pivot": [1.0]}
    elif name == "equal_pivots":
        M, r, base = [[2.0, 0.0, 1.0], [-2.0, 1.0, 0.0], [1.0, 0.0, 1.0]], [3.0, -1.0, 2.0], [0.5, 0.25, 0.0]  # |2| = |-2|: row 0 stays
        expect = {"status": [1], "delta": [[1.0, 1.0, 1.0]], "min_pivot": [0.5]}
    elif name == "last_exchange":
        M, r, base = [[1.0, 0.0, 0.0], [0.0, 0.5, 1.0], [0.0, 2.0, 0.0]], [1.0, 2.5, 2.0], [0.5, 0.25, 0.0]  # rows 1 and 2 at k = 1
        expect = {"status": [1], "delta": [[1.0, 1.0, 2.0]], "min_pivot": [1.0]}
    elif name == "singular":
        M = [[0.0, 1.0], [0.0, 2.0]]                        # J = I in column 0
        expect = {"status": [3], "base_unchanged": True, "min_pivot": [0.0]}
    elif name == "damping":
        kw["damping"] = 0.5
        M, r = [[2.0, 0.0], [0.0, 4.0]], [1.0, 1.0]
        expect = {"status": [1], "delta": [[0.5, 0.25]], "base": [[0.75, -0.125]]}
    elif name in ("converged", "converged_switch_mismatch"):
        r = [0.0, 0.0]
        expect = {"status": [0], "base_unchanged": True} if name == "converged" else {"status": [1], "delta": [[0.0, 0.0]], "n_switch_mismatch": [1.0]}
    elif name == "nan_perturbed":
        expect = {"status": [4], "base_unchanged": True}
    elif name == "nominal_singular":
        ist, expect = [1, 0, 0], {"status": [2], "base_unchanged": True}
    elif name == "perturbed_singular":
        ist, expect = [0, 0, 1], {"status": [4], "base_unchanged": True}
    elif name == "stopped":
        ist, expect = [0, -1, 0], {"status": [5], "base_unchanged": True}
    nX = len(r)
    kinds = (nX, 0, 0)
    method = abi.PSS_SETTLE if name == "settle" else abi.PSS_NEWTON
    n_ckt = 2 if name == "done_beside" else 1
    req = abi.pss_req(n_ckt, method, rel_step=H2, **kw)
    base = np.tile(np.asarray(base, float), (n_ckt, 1))
    base_on = np.ones((n_ckt, nS), np.int32)
    if name == "h_representable":
        req = abi.pss_req(1)
        base = np.array([[1.0 / 3.0, 3.0e-7]])
        X, on, h = pss.design_reference_pss(base, base_on, kinds, method, req.rel_step, req.v_scale, req.i_scale)
        expect = {"h": h, "h_is_not_the_step": True}
        return dict(kinds=kinds, req=req, base=base, base_on=base_on, h=h, X=X, on=on, done=np.zeros(1, np.int32), ist=None, expect=expect)
    if method == abi.PSS_SETTLE:
        X = base + np.asarray(r)[None, :]
        h = None
        expect = {"status": [1], "delta": [r], "base": X.copy()}
    else:
        X = np.concatenate([_dyadic(M, r, base[c]) for c in range(n_ckt)])
        h = np.full((n_ckt, nX), H2)
    on = np.ones((len(X), nS), np.int32)
    if name == "converged_switch_mismatch":
        on[0, 0] = 0
    if name == "nan_perturbed":
        X[2, 1] = np.nan
    done = np.zeros(n_ckt, np.int32)
    if name == "done_beside":
        done[0] = 1
        expect = {"status": [SENTINEL, 1], "delta": [[SENTINEL, SENTINEL], [0.5, -0.5]]}
    return dict(kinds=kinds, req=req, base=base, base_on=base_on, h=h, X=X, on=on, done=done, ist=ist, expect=expect)
