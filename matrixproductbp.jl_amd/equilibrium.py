"""Equilibrium observables of the Ising model on infinite diluted graphs (reference src/Models/glauber/equilibrium.jl):
what the plateau of a long Glauber run (`mpbp_infinite_graph` with Glauber factors) is compared against.

`equilibrium_observables` is the closed-form fixed point on a random regular graph: host arithmetic, no library, no GPU.
`equilibrium_magnetization` is population dynamics on the device (C ABI: mpbp_popdyn_* in include/mpbp_hip.h); like the
rest of the package it raises `MPBPError` without the library or a GPU.

Deliberate differences from the reference:
  * a sweep is synchronous, old array -> new array; the reference updates one array in place in shuffled order and
    alternates between two.  The fixed-point distribution is the same, the trajectory towards it is not;
  * draws are counter based (Philox4x32-10, `seed`) and reproducible; the reference uses Julia's GLOBAL_RNG;
  * only `Dirac`, `Poisson`, `Discrete` and `Normal` are accepted where the reference takes any `Distribution`:
    anything else raises `TypeError`;
  * `equilibrium_energy` (equilibrium.jl:37-40) refers to undefined names in the reference and is not ported;
  * there is no `Measurement`: the result is `(m_avg, m_std)`, the shape `mean_with_uncertainty` returns.
"""
from __future__ import annotations

import ctypes as C
import math
import warnings
from collections import namedtuple

import numpy as np

from . import _lib
from ._lib import MPBPError

DIRAC, DISCRETE, NORMAL = 0, 1, 2          # MPBP_POPDYN_DIRAC ... in include/mpbp_hip.h
PKM1, PK, PJ, PH = 0, 1, 2, 3              # MPBP_POPDYN_PKM1 ...
MAX_TABLE = 256

EquilibriumObservables = namedtuple("EquilibriumObservables", ["m", "r", "e"])


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


class RandomRegular:
    """`RandomRegular(k)` (equilibrium.jl:4-6)"""

    def __init__(self, k):
        self.k = int(k)

    def __repr__(self):
        return f"RandomRegular({self.k})"


class ErdosRenyi:
    """`ErdosRenyi(c)`, c the mean connectivity (equilibrium.jl:8-10)"""

    def __init__(self, c):
        self.c = float(c)

    def __repr__(self):
        return f"ErdosRenyi({self.c})"


# ------------------------------------------------------------------------------------------------ distributions
# plain containers; `table()` -> (kind, values, cdf) in the form mpbp_popdyn_set_distribution takes (cdf None if unused)
class Dirac:
    def __init__(self, value):
        self.value = float(value)

    def table(self):
        return DIRAC, np.array([self.value]), None


class Normal:
    def __init__(self, mu=0.0, sigma=1.0):
        self.mu, self.sigma = float(mu), float(sigma)
        if not self.sigma >= 0:
            raise ValueError(f"Normal: sigma = {sigma} must not be negative")

    def table(self):
        return NORMAL, np.array([self.mu, self.sigma]), None


class Discrete:
    """values[j] with probability probs[j]; the cdf is the running sum of probs, its last entry set to exactly 1"""

    def __init__(self, values, probs):
        self.values = np.ascontiguousarray(values, dtype=np.float64).ravel()
        self.probs = np.ascontiguousarray(probs, dtype=np.float64).ravel()
        if self.values.size != self.probs.size or self.values.size < 1:
            raise ValueError("Discrete: values and probs must have the same non-zero length")
        if self.values.size > MAX_TABLE:
            raise ValueError(f"Discrete: at most {MAX_TABLE} entries (got {self.values.size})")
        if not np.all(np.isfinite(self.probs)) or np.any(self.probs < 0):
            raise ValueError("Discrete: probabilities must be finite and non-negative")
        if abs(float(self.probs.sum()) - 1.0) > 1e-12:
            raise ValueError(f"Discrete: probabilities sum to {float(self.probs.sum())!r}, not 1")

    def table(self):
        cdf = np.cumsum(self.probs)
        cdf[-1] = 1.0
        return DISCRETE, self.values.copy(), np.maximum.accumulate(cdf)


class Poisson:
    """Poisson(c), tabulated as a discrete distribution on 0..K with K the first k whose upper tail P(X > k) is below
    2^-53; more than 256 entries is refused (c of about 140 and above)."""

    def __init__(self, c):
        self.c = float(c)
        if not (self.c >= 0 and math.isfinite(self.c)):
            raise ValueError(f"Poisson: c = {c} must be finite and non-negative")

    def table(self):
        c = self.c
        pmf = [math.exp(-c)]                     # p_k = p_{k-1} c / k
        while True:
            k = len(pmf) - 1
            if k + 1 > c:
                # the upper tail beyond k: past the mode its terms fall at least geometrically, so sum until they vanish
                tail, term, j = 0.0, pmf[-1], k
                while True:
                    j += 1
                    term *= c / j
                    tail += term
                    if term <= tail * 2.0 ** -60:
                        break
                if tail < 2.0 ** -53:
                    break
            if len(pmf) >= MAX_TABLE:
                raise ValueError(f"Poisson({c}): the table needs more than {MAX_TABLE} entries")
            pmf.append(pmf[-1] * c / (k + 1))
        # the last entry takes the tail (a draw falls back on it anyway), so the cdf ends at exactly 1
        cdf = np.minimum(np.cumsum(np.array(pmf)), 1.0)
        cdf[-1] = 1.0
        return DISCRETE, np.arange(len(pmf), dtype=np.float64), cdf


def _table(d, what):
    if not isinstance(d, (Dirac, Poisson, Discrete, Normal)):
        raise TypeError(f"{what}: expected Dirac, Poisson, Discrete or Normal, got {type(d).__name__}")
    return d.table()


# ------------------------------------------------------------------------------------------------ closed form
def iterate_fixedpoint(f, init, maxiter=1000, atol=0, rtol=1e-16, damp=0.0):
    """`iterate_fixedpoint` (equilibrium.jl:12-23)"""
    x = init
    err = math.inf
    for _ in range(maxiter):
        xnew = f(x)
        err = abs(x - xnew)
        if err <= max(atol, rtol * max(abs(x), abs(xnew))):
            return x
        x = (1 - damp) * xnew + damp * x
    warnings.warn(f"Fixed point iterations did not converge. err={err}", RuntimeWarning, stacklevel=2)
    return x


def equilibrium_observables(g: RandomRegular, J, beta=1.0, h=0.0, maxiter=1000, tol=1e-16, init=None, damp=0.0):
    """`equilibrium_observables(g::RandomRegular, J; β, h, ...)` (equilibrium.jl:25-34): magnetisation m, nearest-
    neighbour correlation r and energy per spin e at the fixed point of the cavity field."""
    if not isinstance(g, RandomRegular):
        raise TypeError(f"equilibrium_observables is defined for RandomRegular, got {type(g).__name__}")
    k = g.k
    if init is None:
        init = 100.0 * (float(np.sign(h)) + float(np.random.random()))
    tJ = math.tanh(beta * J)

    def f(u):
        return (k - 1) / beta * math.atanh(math.tanh(beta * u) * tJ) + h

    ustar = iterate_fixedpoint(f, init, maxiter=maxiter, rtol=tol, atol=tol, damp=damp)
    m = math.tanh(beta * (h + (ustar - h) * k / (k - 1)))
    r = (1 + math.tanh(beta * ustar) ** 2 / tJ) / (1 / tJ + math.tanh(beta * ustar) ** 2)
    e = -k / 2 * J * r - m * h
    return EquilibriumObservables(m=m, r=r, e=e)


# ------------------------------------------------------------------------------------------------ population dynamics
class PopDyn:
    """A population of cavity fields on the device (`mpbp_popdyn`).  Sweeps and draws are a function of `seed` and of
    how many sweeps / draws came before, not of how the calls are split."""

    def __init__(self, P, beta=1.0, seed=0, device=0):
        P = np.ascontiguousarray(P, dtype=np.float64).ravel()
        self.popsize = int(P.size)
        self._L = L = _lib.lib()
        h = C.c_void_p()
        _lib.check(L.mpbp_popdyn_create(C.byref(h), int(device), self.popsize, C.c_uint64(int(seed) & (2 ** 64 - 1)),
                                        float(beta), _dp(P) if P.size else None))
        self._h = h

    def __del__(self):
        try:
            if getattr(self, "_h", None):
                self._L.mpbp_popdyn_destroy(self._h)
                self._h = None
        except Exception:
            pass

    def set_distribution(self, which, dist):
        kind, values, cdf = _table(dist, ("pkm1", "pk", "pJ", "ph")[which])
        self.set_table(which, kind, values, cdf)

    def set_table(self, which, kind, values, cdf=None):
        values = np.ascontiguousarray(values, dtype=np.float64)
        cdf = None if cdf is None else np.ascontiguousarray(cdf, dtype=np.float64)
        _lib.check(self._L.mpbp_popdyn_set_distribution(self._h, int(which), int(kind), int(values.size), _dp(values),
                                                        None if cdf is None else _dp(cdf)))

    def iterate(self, nsweeps=1):
        """`nsweeps` sweeps queued on the device; returns the mean of the population after each"""
        means = np.zeros(max(int(nsweeps), 0))
        _lib.check(self._L.mpbp_popdyn_iterate(self._h, int(nsweeps), _dp(means) if means.size else None))
        return means

    def get_population(self):
        P = np.zeros(self.popsize)
        _lib.check(self._L.mpbp_popdyn_get_population(self._h, _dp(P)))
        return P

    def set_population(self, P):
        P = np.ascontiguousarray(P, dtype=np.float64).ravel()
        if P.size != self.popsize:
            raise ValueError(f"set_population: expected {self.popsize} values, got {P.size}")
        _lib.check(self._L.mpbp_popdyn_set_population(self._h, _dp(P)))

    def magnetization(self, nsamples):
        m = np.zeros(max(int(nsamples), 0))
        _lib.check(self._L.mpbp_popdyn_magnetization(self._h, int(nsamples), _dp(m) if m.size else None))
        return m


class CB_Pop:
    """`CB_Pop` (equilibrium.jl:43-69) without the progress bar: `.m` holds the statistic at every check (starting
    `[inf]`), `.Δs` its change.  With `f=None` the statistic is the mean of the population, reduced on the device.  A user
    `f` is the slow path: the whole population is downloaded at every check and `f(P)` is called on it."""

    def __init__(self, f=None):
        self.f = f
        self.m = [math.inf]
        self.Δs = []

    def __call__(self, stat, it, maxiter, tol):
        mnew = float(stat)
        d = abs(mnew - self.m[-1])
        self.Δs.append(d)
        self.m.append(mnew)
        return d


def equilibrium_magnetization(g_or_pkm1, pk=None, *, pJ=Dirac(1.0), beta=1.0, ph=Dirac(0.0), popsize=1000, maxiter=1000,
                              tol=None, nsamples=1000, seed=0, P=None, cb=None, check_every=1):
    """`equilibrium_magnetization` (equilibrium.jl:72-127) -> `(m_avg, m_std)`, m_avg = |mean(m)| and m_std = std(m) /
    sqrt(nsamples) over `nsamples` draws from the converged population.

    `RandomRegular(k)` stands for pkm1 = Dirac(k-1), pk = Dirac(k); `ErdosRenyi(c)` for Poisson(c) twice; otherwise pass
    the residual degree distribution `pkm1` and the degree profile `pk`.  `P` defaults to `popsize` standard normals of
    `numpy.random.default_rng(seed)`.  Every `check_every` sweeps the callback gets the statistic (`CB_Pop`); the run
    stops once its change falls below `tol` (default 0.1 / sqrt(popsize)) and warns if `maxiter` sweeps did not get there."""
    if isinstance(g_or_pkm1, RandomRegular):
        if pk is not None:
            raise TypeError("equilibrium_magnetization(RandomRegular(k)) takes no pk")
        pkm1, pk = Dirac(g_or_pkm1.k - 1), Dirac(g_or_pkm1.k)
    elif isinstance(g_or_pkm1, ErdosRenyi):
        if pk is not None:
            raise TypeError("equilibrium_magnetization(ErdosRenyi(c)) takes no pk")
        pkm1, pk = Poisson(g_or_pkm1.c), Poisson(g_or_pkm1.c)
    else:
        pkm1 = g_or_pkm1
        if pk is None:
            raise TypeError("equilibrium_magnetization(pkm1, pk): the degree profile pk is missing")
    tables = [_table(d, nm) for d, nm in ((pkm1, "pkm1"), (pk, "pk"), (pJ, "pJ"), (ph, "ph"))]
    if P is None:
        P = np.random.default_rng(seed).standard_normal(int(popsize))
    P = np.ascontiguousarray(P, dtype=np.float64).ravel()
    if tol is None:
        tol = 0.1 / math.sqrt(P.size)
    check_every = int(check_every)
    if check_every < 1:
        raise ValueError(f"check_every must be positive (got {check_every})")
    if cb is None:
        cb = CB_Pop()
    user_f = getattr(cb, "f", None)

    pop = PopDyn(P, beta=beta, seed=seed)
    for which, (kind, values, cdf) in enumerate(tables):
        pop.set_table(which, kind, values, cdf)
    delta, it = math.inf, 0
    while it < maxiter:
        n = min(check_every, maxiter - it)
        means = pop.iterate(n)
        it += n
        stat = means[-1] if user_f is None else user_f(pop.get_population())
        delta = cb(stat, it, maxiter, tol)
        if delta < tol:
            break
    if not delta < tol:
        warnings.warn(f"Population dynamics did not converge. Error {delta}", RuntimeWarning, stacklevel=2)
    m = pop.magnetization(int(nsamples))
    m_avg = abs(float(np.mean(m)))
    m_std = float(np.std(m, ddof=1)) / math.sqrt(m.size) if m.size > 1 else 0.0
    return m_avg, m_std
