"""Exact solvers on the device (reference src/exact.jl; C ABI: mpbp_exact_* in include/mpbp_hip.h): the ground truth an
MPBP run is compared against.

Two methods.  `"enumerate"` is the reference's: the probability of every one of the Q = prod_i q_i^(T+1) trajectories
(Q <= 2^32), from which every `exact_*` quantity follows.  `"transfer"` is a forward-backward recursion over the joint
state of all nodes at one time (S = prod_i q_i <= 2^16 states): exact on any graph, loopy or not, at ANY T - it gives
log Z, marginals, same-time pair marginals and, through `ExactSolver.twovar_marginals` / `.alternate_twovar_marginals`, the
two-time and alternate marginals; not the joint.  `"auto"` enumerates when Q <= 2^26, else transfers.  The module functions
for two-time quantities (`exact_beliefs_tu`, `exact_autocorrelations`, `exact_autocovariances`, `exact_alternate_marginals`)
enumerate wherever that is possible and go to a transfer solver only where enumeration is refused for size.

Layout of `p`: a C-ordered array of shape `[q_0]*(T+1) + [q_1]*(T+1) + ...` (node-major, time inside), 0-based states.
Functions `f` receive 1-based states, as everywhere in this package.  The reference's bare `pair_marginals(bp; p)` is
`ExactSolver.edge_marginals()` here: `sampling.pair_marginals` owns that name.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import MPBPError
from .mpbp import MPBP, _abi_maxdist, _dp, _ip

ENUM_AUTO_MAX = 1 << 26       # "auto" enumerates up to this many configurations
ENUM_MAX = 1 << 32
ENUM_MAX_DIGITS = 64
TRANSFER_MAX = 1 << 16
_METHODS = {"enumerate": 0, "transfer": 1}


def choose_method(qnode, T, periodic=False):
    """The `"auto"` rule: `"enumerate"` when Q = prod_i q_i^(T+1) <= 2^26, otherwise `"transfer"` where that is admissible
    (S = prod_i q_i <= 2^16, q <= 4, chains not periodic in time); otherwise MPBPError(-4)."""
    qn = [int(v) for v in qnode]
    Q = 1
    for v in qn:
        Q *= v ** (int(T) + 1)
    if Q <= ENUM_AUTO_MAX and len(qn) * (int(T) + 1) <= ENUM_MAX_DIGITS and max(qn) <= 4:
        return "enumerate"
    S = 1
    for v in qn:
        S *= v
    if S <= TRANSFER_MAX and max(qn) <= 4 and not periodic:
        return "transfer"
    raise MPBPError(-4, f"no exact method for this size: Q = {Q} configurations exceed 2^26 and the global-state transfer "
                        f"needs S = {S} <= 2^16, q <= 4 and chains that are not periodic in time")


class ExactSolver:
    """`ExactSolver(bp, method="auto" | "enumerate" | "transfer")`.  A solver is a snapshot of `bp`: what it has downloaded
    is cached, so make a new one after changing `bp`'s observations or factors."""

    def __init__(self, bp: MPBP, method="auto"):
        if method == "auto":
            method = choose_method(bp.qnode, bp.T, bp.periodic)
        if method not in _METHODS:
            raise ValueError(f"method must be 'auto', 'enumerate' or 'transfer', got {method!r}")
        self.bp, self.method = bp, method
        self._cache = {}
        self._h = None
        h = C.c_void_p()
        L = bp._L
        _lib.check(L.mpbp_exact_create(C.byref(h), bp._h, _METHODS[method]), bp._h)
        self._h, self._L = h, L

    def __del__(self):
        try:
            if getattr(self, "_h", None):
                self._L.mpbp_exact_destroy(self._h)
                self._h = None
        except Exception:
            pass

    def _check(self, rc):
        _lib.check(rc, self.bp._h)

    def _shape(self, nodes):
        L = self.bp.T + 1
        return tuple(int(self.bp.qnode[i]) for i in nodes for _ in range(L))

    # --- solve ----------------------------------------------------------------------------------
    @property
    def logZ(self):
        if "logZ" not in self._cache:
            z = C.c_double()
            self._check(self._L.mpbp_exact_solve(self._h, C.byref(z)))
            self._cache["logZ"] = float(z.value)
        return self._cache["logZ"]

    @property
    def Z(self):
        return float(np.exp(self.logZ))

    def set_prob(self, p):
        """Loads a `p` returned by `exact_prob` / `.prob()`: the marginals are then reductions of it (no solve)."""
        p = np.ascontiguousarray(p, dtype=np.float64)
        if p.shape != self._shape(range(self.bp.g.nv())):
            raise MPBPError(-1, f"p has shape {p.shape}, this model's joint has {self._shape(range(self.bp.g.nv()))}")
        self._check(self._L.mpbp_exact_set_prob(self._h, _dp(p)))
        self._cache = {"p": p}
        return self

    def prob(self):
        """`exact_prob(bp)[1]` (src/exact.jl:5-41): p of every trajectory, in the layout of the module docstring."""
        if "p" not in self._cache:
            shape = self._shape(range(self.bp.g.nv()))
            if self.method == "enumerate":
                self.logZ                                   # solve first: the host array is only made once that worked
            p = np.zeros(shape if self.method == "enumerate" else 1)
            self._check(self._L.mpbp_exact_prob(self._h, _dp(p)))
            self._cache["p"] = p
        return self._cache["p"]

    # --- marginals ------------------------------------------------------------------------------
    def marginals(self):
        """`exact_marginals` (src/exact.jl:60-74): `out[i][t][x]`"""
        if "m" not in self._cache:
            bp = self.bp
            N, L, q = bp.g.nv(), bp.T + 1, bp.q
            buf = np.zeros(q * L * N)
            self._check(self._L.mpbp_exact_marginals(self._h, _dp(buf)))
            m = buf.reshape((q, L, N), order="F")
            self._cache["m"] = [[m[:bp.qnode[i], t, i].copy() for t in range(L)] for i in range(N)]
        return self._cache["m"]

    def pair_marginals(self):
        """`exact_pair_marginals` (src/exact.jl:102-119): `out[e][t][x_i, x_j]` per directed edge e = (i -> j)"""
        if "pm" not in self._cache:
            bp = self.bp
            E, L, q = bp.g.ne(), bp.T + 1, bp.q
            buf = np.zeros(q * q * L * E)
            self._check(self._L.mpbp_exact_pair_marginals(self._h, _dp(buf)))
            m = buf.reshape((q, q, L, E), order="F")
            ends = bp._ends
            self._cache["pm"] = [[m[:bp.qnode[ends[e][0]], :bp.qnode[ends[e][1]], t, e].copy() for t in range(L)]
                                 for e in range(E)]
        return self._cache["pm"]

    def site_marginals(self):
        """`site_marginals(bp; p)` (src/exact.jl:43-58): per node the marginal of its whole trajectory, shape [q_i]*(T+1)"""
        if "site" not in self._cache:
            out = []
            for i in range(self.bp.g.nv()):
                a = np.zeros(self._shape([i]) if self.method == "enumerate" else 1)
                self._check(self._L.mpbp_exact_site_marginals(self._h, i, _dp(a)))
                out.append(a)
            self._cache["site"] = out
        return self._cache["site"]

    def edge_marginals(self):
        """The reference's exact `pair_marginals(bp; p)` (src/exact.jl:85-100): per directed edge (i -> j) the joint of the
        two trajectories, shape [q_i]*(T+1) + [q_j]*(T+1)"""
        if "edge" not in self._cache:
            out = []
            for (i, j, e) in self.bp.g.edges():
                a = np.zeros(self._shape([i, j]) if self.method == "enumerate" else 1)
                self._check(self._L.mpbp_exact_edge_marginals(self._h, e, _dp(a)))
                out.append(a)
            self._cache["edge"] = out
        return self._cache["edge"]

    def alternate_marginals(self):
        """`exact_alternate_marginals` (src/exact.jl:132-148): `out[e][t][x_i^t, x_j^{t+1}]`, t < T, as axis sums of
        `edge_marginals()` (enumeration only).  The form for both methods, at any T: `alternate_twovar_marginals()`."""
        if "alt" not in self._cache:
            L = self.bp.T + 1
            out = []
            for m in self.edge_marginals():
                out.append([m.sum(axis=tuple(a for a in range(2 * L) if a not in (t, L + t + 1))) for t in range(L - 1)])
            self._cache["alt"] = out
        return self._cache["alt"]

    def autocorrelations(self, f=None):
        """`exact_autocorrelations(f, bp)` (src/exact.jl:161-186): `out[i][t, u]` = E[f(x_i^t, i) f(x_i^u, i)], t < u, from
        `site_marginals()` (enumeration only).  The form for both methods, at any T: `twovar_autocorrelations(f)`, built
        on `twovar_marginals()`."""
        f = (lambda x, i: x) if f is None else f
        L = self.bp.T + 1
        out = []
        for i, m in enumerate(self.site_marginals()):
            fx = np.array([f(x + 1, i) for x in range(m.shape[0])], dtype=float)
            r = np.zeros((L, L))
            for u in range(L):
                for t in range(u):
                    p = m.sum(axis=tuple(a for a in range(L) if a not in (t, u)))
                    r[t, u] = fx @ p @ fx
            out.append(r)
        return out

    # --- two-time quantities on both methods (mpbp_exact_twovar_marginals / mpbp_exact_alternate_marginals) -----------
    def _twovar_raw(self, sites, maxdist):
        bp = self.bp
        L, q = bp.T + 1, bp.q
        nodes = np.ascontiguousarray(sites, dtype=np.int32)
        buf = np.zeros(len(sites) * L * L * q * q)
        md = _abi_maxdist(maxdist)
        if md >= 0 and len(sites) > 0:       # maxdist = 0: no pair at all, no library call (the ABI's 0 means "all")
            self._check(self._L.mpbp_exact_twovar_marginals(self._h, _ip(nodes), int(nodes.size), md, _dp(buf)))
        return buf.reshape((len(sites), L, L, q, q))           # [k][t][u][y][x]

    def twovar_marginals(self, sites=None, maxdist=None):
        """Exact two-time marginals in the shape of `beliefs_tu`: `out[k][t][u][x_t, x_u]`, a q_i x q_i array for
        t < u <= t + maxdist and None elsewhere, for the listed nodes (all by default).  Enumeration: strided reductions
        of p; transfer: conditioned vectors carried through the transfer matrix, at any T.  Nothing is cached."""
        bp = self.bp
        sites = list(range(bp.g.nv())) if sites is None else [int(i) for i in sites]
        L = bp.T + 1
        arr = self._twovar_raw(sites, maxdist)
        md = L if maxdist is None else int(maxdist)
        qs = [int(bp.qnode[i]) if 0 <= i < bp.g.nv() else bp.q for i in sites]
        return [[[arr[k, t, u, :qs[k], :qs[k]].T.copy() if t < u <= t + md else None for u in range(L)] for t in range(L)]
                for k in range(len(sites))]

    def twovar_autocorrelations(self, f=None, sites=None, maxdist=None):
        """`out[k][t, u]` = E[f(x_i^t, i) f(x_i^u, i)] for t < u <= t + maxdist (0 elsewhere), from `twovar_marginals`"""
        f = (lambda x, i: x) if f is None else f
        bp = self.bp
        sites = list(range(bp.g.nv())) if sites is None else [int(i) for i in sites]
        arr = self._twovar_raw(sites, maxdist)
        out = []
        for k, i in enumerate(sites):
            fx = np.array([f(x + 1, i) if x < bp.qnode[i] else 0.0 for x in range(bp.q)], dtype=float)
            out.append(np.einsum("tuyx,x,y->tu", arr[k], fx, fx))
        return out

    def alternate_twovar_marginals(self):
        """`out[e][t][x_i^t, x_j^{t+1}]`, t < T, per directed edge e = (i -> j), on both methods and at any T"""
        bp = self.bp
        E, T, q = bp.g.ne(), bp.T, bp.q
        buf = np.zeros(q * q * T * E)
        if buf.size:
            self._check(self._L.mpbp_exact_alternate_marginals(self._h, _dp(buf)))
        m = buf.reshape((q, q, T, E), order="F")
        ends = bp._ends
        return [[m[:bp.qnode[ends[e][0]], :bp.qnode[ends[e][1]], t, e].copy() for t in range(T)] for e in range(E)]


def _solver(bp, p_exact, method):
    if isinstance(p_exact, ExactSolver):
        return p_exact
    if p_exact is None:
        return ExactSolver(bp, method)
    return ExactSolver(bp, "enumerate").set_prob(p_exact)


def exact_prob(bp: MPBP):
    """`exact_prob(bp)` (src/exact.jl:5-41): `(p, Z)`"""
    s = ExactSolver(bp, "enumerate")
    return s.prob(), s.Z


def site_marginals(bp: MPBP, p=None):
    """src/exact.jl:43-58"""
    return _solver(bp, p, "enumerate").site_marginals()


def exact_marginals(bp: MPBP, p_exact=None):
    """src/exact.jl:60-74: `out[i][t][x]`"""
    return _solver(bp, p_exact, "auto").marginals()


def exact_pair_marginals(bp: MPBP, p_exact=None):
    """src/exact.jl:102-119: `out[e][t][x_i, x_j]`"""
    return _solver(bp, p_exact, "auto").pair_marginals()


def _twotime_solver(bp, p_exact):
    """The solver behind the two-time module functions: today's route, enumeration, wherever it works; a transfer solver
    only where enumeration is refused for size (MPBPError -4).  A solver that is passed in is used as it is."""
    if p_exact is not None:
        return _solver(bp, p_exact, "enumerate")
    try:
        return ExactSolver(bp, "enumerate")
    except MPBPError as e:
        if e.code != -4:
            raise
        return ExactSolver(bp, "transfer")


def exact_beliefs_tu(bp: MPBP, sites=None, maxdist=None, p_exact=None):
    """The exact counterpart of `beliefs_tu`: `out[k][t][u][x_t, x_u]` for t < u <= t + maxdist, None elsewhere"""
    return _twotime_solver(bp, p_exact).twovar_marginals(sites, maxdist)


def exact_alternate_marginals(bp: MPBP, p_exact=None):
    """src/exact.jl:132-148: `out[e][t][x_i^t, x_j^{t+1}]`"""
    s = _twotime_solver(bp, p_exact)
    return s.alternate_marginals() if s.method == "enumerate" else s.alternate_twovar_marginals()


def exact_autocorrelations(*args, p_exact=None, maxdist=None):
    """`exact_autocorrelations(f, bp)` or `exact_autocorrelations(bp)` with f(x, i) = x (src/exact.jl:161-188); with
    `maxdist`, entries beyond t + maxdist are 0 as in `autocorrelations`"""
    f, bp = _f_bp(args)
    s = _twotime_solver(bp, p_exact)
    if s.method != "enumerate":
        return s.twovar_autocorrelations(f, maxdist=maxdist)
    r = s.autocorrelations(f)
    if maxdist is not None:
        L = bp.T + 1
        keep = np.array([[t < u <= t + int(maxdist) for u in range(L)] for t in range(L)])
        r = [np.where(keep, ri, 0.0) for ri in r]
    return r


def exact_autocovariances(*args, r=None, mu=None, p_exact=None, maxdist=None):
    """src/exact.jl:191-198: `covariance(r, mu) = r - mu mu'` (src/mpbp.jl:288)"""
    f, bp = _f_bp(args)
    if r is None or mu is None:
        p_exact = _twotime_solver(bp, p_exact)
    r = exact_autocorrelations(f, bp, p_exact=p_exact, maxdist=maxdist) if r is None else r
    mu = exact_marginal_expectations(f, bp, p_exact=p_exact) if mu is None else mu
    return [ri - np.outer(mi, mi) for ri, mi in zip(r, mu)]


def _f_bp(args):
    if len(args) == 1:
        return (lambda x, i: x), args[0]
    if len(args) == 2:
        return args
    raise TypeError("expected (bp) or (f, bp)")


def _expect(fx, p):
    """`expectation(f, p)` (src/mpbp.jl:241-243): sum f(x) p[x], or sum f(x) f(y) p[x, y] for a matrix"""
    p = np.asarray(p)
    return float(fx[:p.shape[0]] @ p) if p.ndim == 1 else float(fx[:p.shape[0]] @ p @ fx[:p.shape[1]])


def _expectations(f, bp, tables):
    fx = lambda i: np.array([f(x + 1, i) for x in range(bp.q)], dtype=float)
    return [np.array([_expect(fx(i), m) for m in mi]) for i, mi in enumerate(tables)]


def exact_marginal_expectations(*args, m_exact=None, p_exact=None):
    """src/exact.jl:76-83: `out[i][t]` = E[f(x_i^t, i)]"""
    f, bp = _f_bp(args)
    return _expectations(f, bp, exact_marginals(bp, p_exact) if m_exact is None else m_exact)


def exact_pair_marginal_expectations(*args, m_exact=None, p_exact=None):
    """src/exact.jl:121-130: `out[e][t]` = E[f(x_i^t, e) f(x_j^t, e)] - f is indexed by the EDGE, as in the reference"""
    f, bp = _f_bp(args)
    return _expectations(f, bp, exact_pair_marginals(bp, p_exact) if m_exact is None else m_exact)


def exact_alternate_marginal_expectations(*args, m_exact=None, p_exact=None):
    """src/exact.jl:150-158: `out[e][t]` = E[f(x_i^t, e) f(x_j^{t+1}, e)] (at any T where enumeration is refused for size)"""
    f, bp = _f_bp(args)
    return _expectations(f, bp, exact_alternate_marginals(bp, p_exact) if m_exact is None else m_exact)
