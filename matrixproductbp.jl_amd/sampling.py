"""SoftMargin importance sampler (reference src/sampling.jl): trajectories drawn on the device from the prior dynamics of
an `MPBP`'s factors, weighted by its observations `phi^{t>=1}` and pair potentials `psi` (C ABI: mpbp_sampler_* in
include/mpbp_hip.h).

States of returned trajectories are 1-based, as `logprob` expects; node, edge and time indices are 0-based, as
everywhere else in this package.  `Measurement`s do not exist here: marginals and observables come as `(value, err)`.

One deliberate difference from the reference: it stores `exp(logl)` as a Float64, so weights underflow to 0 once
log w < -745; here log-weights are kept throughout (`.logw`) and the device accumulates exp(log w - M) with M the running
maximum.
"""
from __future__ import annotations

import ctypes as C
import warnings

import numpy as np

from . import _lib
from ._lib import MPBPError
from .mpbp import MPBP, InfiniteBipartiteRegularGraph, InfiniteRegularGraph, _dp, _ip


class SoftMarginSampler:
    """`SoftMarginSampler` (src/sampling.jl:5-28).  The draws are a function of `(seed, sample index)` only: sampling
    300 then 700 gives the trajectories of sampling 1000.  `keep_samples=True` keeps the trajectories in `.X` (list of
    1-based `[N, T+1]` arrays); `.logw` always holds the log-weights.  Two-time joints (for `autocorrelations`) are
    accumulated for `autocorr_sites` only, up to `maxdist` (None: all distances)."""

    def __init__(self, bp: MPBP, seed=0, keep_samples=False, autocorr_sites=None, maxdist=None):
        if isinstance(bp.g, (InfiniteRegularGraph, InfiniteBipartiteRegularGraph)):
            raise MPBPError(-4, "sampling needs an explicit graph: a trajectory of the k aliased copies of one node of "
                                f"{type(bp.g).__name__} has no meaning")
        self.bp, self.seed, self.keep_samples = bp, int(seed), bool(keep_samples)
        self.X, self.logw = [], np.zeros(0)
        T = bp.T
        self.sites = [] if autocorr_sites is None else [int(i) for i in autocorr_sites]
        self.maxdist = T if maxdist is None else int(maxdist)
        if self.sites and not 1 <= self.maxdist <= T:
            raise ValueError(f"invalid maxdist {maxdist}: need 1 <= maxdist <= T = {T}")
        sites = np.ascontiguousarray(self.sites if self.sites else [0], dtype=np.int32)
        h = C.c_void_p()
        L = bp._L
        _lib.check(L.mpbp_sampler_create(C.byref(h), bp._h, C.c_uint64(self.seed & (2 ** 64 - 1)), _ip(sites),
                                         len(self.sites), self.maxdist), bp._h)
        self._h, self._L = h, L

    def __del__(self):
        try:
            if getattr(self, "_h", None):
                self._L.mpbp_sampler_destroy(self._h)
                self._h = None
        except Exception:
            pass

    @property
    def nsamples(self):
        n = C.c_int64()
        self._check(self._L.mpbp_sampler_counts(self._h, C.byref(n), None, None))
        return int(n.value)

    def _check(self, rc):
        _lib.check(rc, self.bp._h)

    def _sample(self, nsamples):
        nsamples = int(nsamples)
        N, L = self.bp.g.nv(), self.bp.T + 1
        lw = np.zeros(max(nsamples, 0))
        X = np.zeros((max(nsamples, 0), L, N), dtype=np.uint8) if self.keep_samples else None
        xp = X.ctypes.data_as(C.POINTER(C.c_uint8)) if X is not None else None
        self._check(self._L.mpbp_sample(self._h, nsamples, xp, _dp(lw)))
        if X is not None:
            self.X.extend(x.T.astype(np.int64) + 1 for x in X)
        self.logw = np.concatenate([self.logw, lw])
        return self


def sample(obj, nsamples, **kw):
    """`sample(bp, nsamples; kw...)` returns a new sampler (keyword arguments of `SoftMarginSampler`); `sample(sms,
    nsamples)` appends to an existing one - the reference's `sample!` (src/sampling.jl:69-93)."""
    if isinstance(obj, SoftMarginSampler):
        if kw:
            raise TypeError(f"sample(sms, n) takes no keyword arguments, got {sorted(kw)}")
        return obj._sample(nsamples)
    return SoftMarginSampler(obj, **kw)._sample(nsamples)


def onesample(bp: MPBP, seed=0):
    """`onesample(bp)` (src/sampling.jl:30-66): one trajectory `x[i, t]` (1-based states) and its weight w = exp(log w)."""
    sms = sample(bp, 1, seed=seed, keep_samples=True)
    return sms.X[0], float(np.exp(sms.logw[0]))


def effective_sample_size(sms: SoftMarginSampler):
    """(sum w)^2 / sum w^2 of the samples drawn so far."""
    n, a, b = C.c_int64(), C.c_double(), C.c_double()
    sms._check(sms._L.mpbp_sampler_counts(sms._h, C.byref(n), C.byref(a), C.byref(b)))
    return float(np.exp(2 * a.value - b.value)) if np.isfinite(a.value) else 0.0


def _err(p, n):
    return np.sqrt(np.clip(p * (1 - p), 0.0, None) / n)


def marginals(sms: SoftMarginSampler, sites=None):
    """`marginals(sms)` (src/sampling.jl:95-122): `(value, err)`, each `[site][t]` -> array over the node's states;
    err = sqrt(p (1 - p) / nsamples)."""
    bp = sms.bp
    N, L, q = bp.g.nv(), bp.T + 1, bp.q
    buf = np.zeros(q * L * N)
    sms._check(sms._L.mpbp_sampler_marginals(sms._h, _dp(buf)))
    m = buf.reshape((q, L, N), order="F")
    n = sms.nsamples
    sites = range(N) if sites is None else sites
    val = [[m[:bp.qnode[i], t, i].copy() for t in range(L)] for i in sites]
    return val, [[_err(p, n) for p in vi] for vi in val]


def pair_marginals(sms: SoftMarginSampler):
    """`pair_marginals(sms)` (src/sampling.jl:131-153): `(value, err)`, each `[edge][t]` -> q_i x q_j array."""
    bp = sms.bp
    E, L, q = bp.g.ne(), bp.T + 1, bp.q
    buf = np.zeros(q * q * L * E)
    sms._check(sms._L.mpbp_sampler_pair_marginals(sms._h, _dp(buf)))
    m = buf.reshape((q, q, L, E), order="F")
    n = sms.nsamples
    ends = bp._ends
    val = [[m[:bp.qnode[ends[e][0]], :bp.qnode[ends[e][1]], t, e].copy() for t in range(L)] for e in range(E)]
    return val, [[_err(p, n) for p in ve] for ve in val]


def twovar_marginals(sms: SoftMarginSampler):
    """The weighted two-time joints of the sites requested at creation: `[k][t][u]` -> q x q array p(x^t, x^u) for
    t < u <= t + maxdist, else None."""
    if not sms.sites:
        raise ValueError("no autocorr_sites were requested when the sampler was created")
    bp = sms.bp
    L, q = bp.T + 1, bp.q
    buf = np.zeros(len(sms.sites) * L * L * q * q)
    sms._check(sms._L.mpbp_sampler_twovar_marginals(sms._h, _dp(buf)))
    arr = buf.reshape((len(sms.sites), L, L, q, q))          # [k][t][u][y][x], x fastest
    return [[[arr[k, t, u].T.copy() if t < u <= t + sms.maxdist else None for u in range(L)] for t in range(L)]
            for k in range(len(sms.sites))]


def means(f, sms: SoftMarginSampler, sites=None):
    """`means(f, sms)` (src/sampling.jl:124-129): `(value, err)` of E[f(x_i^t, i)] per site and time."""
    N = sms.bp.g.nv()
    sites = list(range(N)) if sites is None else list(sites)
    val, err = marginals(sms, sites)
    mv, me = [], []
    for i, vi, ei in zip(sites, val, err):
        fx = np.array([f(x + 1, i) for x in range(len(vi[0]))], dtype=float)
        mv.append(np.array([fx @ p for p in vi]))
        me.append(np.array([np.sqrt(np.sum((fx * e) ** 2)) for e in ei]))
    return mv, me


def autocorrelations(f, sms: SoftMarginSampler, sites=None, maxdist=None):
    """`autocorrelations(f, sms; sites, maxdist)` (src/sampling.jl:155-183): `(r, err)` per site, (T+1) x (T+1) arrays with
    r[t, u] = E[f(x^t) f(x^u)] for t < u <= t + maxdist (0 elsewhere).  The sites must have been requested when the sampler
    was created (`autocorr_sites`), and maxdist may not exceed the one given there."""
    T = sms.bp.T
    if not sms.sites:
        raise ValueError("autocorrelations of a SoftMarginSampler need autocorr_sites at its creation")
    sites = list(sms.sites) if sites is None else [int(i) for i in sites]
    missing = [i for i in sites if i not in sms.sites]
    if missing:
        raise ValueError(f"sites {missing} were not requested as autocorr_sites when the sampler was created")
    md = sms.maxdist if maxdist is None else int(maxdist)
    if not 1 <= md <= T:
        raise ValueError(f"invalid maxdist {maxdist}: need 1 <= maxdist <= T = {T}")
    if md > sms.maxdist:
        raise ValueError(f"maxdist {md} exceeds the {sms.maxdist} the sampler accumulates")
    tv = twovar_marginals(sms)
    n, L = sms.nsamples, T + 1
    rs, es = [], []
    for i in sites:
        k = sms.sites.index(i)
        qi = sms.bp.qnode[i]
        fx = np.array([f(x + 1, i) for x in range(qi)], dtype=float)
        ff = np.outer(fx, fx)
        r, e = np.zeros((L, L)), np.zeros((L, L))
        for t in range(L):
            for u in range(t + 1, min(L, t + md + 1)):
                p = tv[k][t][u][:qi, :qi]
                r[t, u] = np.sum(ff * p)
                e[t, u] = np.sqrt(np.sum((ff * _err(p, n)) ** 2))
        rs.append(r)
        es.append(e)
    return rs, es


def autocovariances(f, sms: SoftMarginSampler, sites=None, maxdist=None):
    """`autocovariances(f, sms)` (src/sampling.jl:179-185): `covariance(r, mu) = r - mu mu'` (src/mpbp.jl:288) over the
    whole (T+1) x (T+1) matrix, as `mpbp.autocovariances` does - outside the window t < u <= t + maxdist, where r is 0, the
    entry is -mu_t mu_u.  Errors to first order: sqrt(re^2 + (mu_u s_t)^2 + (mu_t s_u)^2) off the diagonal and, the two
    factors being one variable there, 2 |mu_t| s_t on it."""
    sites = list(sms.sites) if sites is None else [int(i) for i in sites]
    r, re = autocorrelations(f, sms, sites, maxdist)
    mu, me = means(f, sms, sites)
    cv, ce = [], []
    for a in range(len(sites)):
        m, s = mu[a], me[a]
        cv.append(r[a] - np.outer(m, m))
        e = np.sqrt(re[a] ** 2 + np.outer(s, m) ** 2 + np.outer(m, s) ** 2)
        np.fill_diagonal(e, 2 * np.abs(m) * s)
        ce.append(e)
    return cv, ce


def mean_with_uncertainty(values, errors):
    """`mean_with_uncertainty` (src/utils.jl:23-35) for independent measurements given as `values` and `errors` (arrays
    of equal shape, measurements along the first axis): (mean, sqrt(sum err^2) / n)."""
    v, e = np.asarray(values, dtype=float), np.asarray(errors, dtype=float)
    return v.mean(axis=0), np.sqrt(np.sum(e ** 2, axis=0)) / v.shape[0]


def draw_node_observations(bp: MPBP, nobs, softinf=np.inf, last_time=False, times=None, rng=None):
    """`draw_node_observations!(bp, nobs; softinf, last_time, times, rng)` (src/sampling.jl:191-210): draws one trajectory
    X from the prior, chooses `nobs` distinct (i, t) pairs among nodes x `times` (default: every time, or only the last
    one if `last_time`), and multiplies phi_i^t by logistic(log softinf) at the drawn state and by logistic(-log softinf)
    elsewhere.  `bp.phi` is updated on the host and on the device.  Returns (X, observed): X 1-based [N, T+1], observed a
    sorted list of 0-based (i, t)."""
    rng = np.random.default_rng() if rng is None else rng
    N, T = bp.g.nv(), bp.T
    X, _ = onesample(bp, seed=int(rng.integers(0, 2 ** 63 - 1)))
    if times is None:
        times = range(T, T + 1) if last_time else range(0, T + 1)
    pairs = [(i, int(t)) for t in times for i in range(N)]
    if nobs > len(pairs):
        raise ValueError(f"nobs = {nobs} exceeds the {len(pairs)} (node, time) pairs")
    pick = rng.choice(len(pairs), size=int(nobs), replace=False)
    observed = sorted(pairs[k] for k in pick)
    with np.errstate(divide="ignore"):
        lsi = np.log(softinf)
    softone, softzero = 1.0 / (1.0 + np.exp(-lsi)), 1.0 / (1.0 + np.exp(lsi))
    for (i, t) in observed:
        qi = bp.qnode[i]
        for x in range(qi):
            bp.phi[x, t, i] *= softone if x == X[i, t] - 1 else softzero
        if np.all(bp.phi[:qi, t, i] == 0):
            warnings.warn(f"Reweighting is giving zero probability to all values of variable {i} at time {t}.")
    _lib.check(bp._L.mpbp_set_phi(bp._h, _dp(np.asfortranarray(bp.phi).ravel(order="F"))), bp._h)
    return X, observed
