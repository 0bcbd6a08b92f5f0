"""Equilibrium Ising observables (reference src/Models/glauber/equilibrium.jl; C ABI mpbp_popdyn_* in include/mpbp_hip.h).

The closed form is checked against values computed independently; the device population dynamics against `HostPop`, a
restatement of the algorithm documented in the header comment of include/mpbp_hip.h (counter layout, distribution tables,
arithmetic order, the reduction tree of the mean) that takes its random words from the library's host entry point
mpbp_philox4x32_10."""
import ctypes as C
import math
import os
import warnings

import numpy as np
import pytest

import mpbp_amd as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E = M.equilibrium
TWO_PI = 6.283185307179586


# ------------------------------------------------------------------------------------------------ host restatement
def tree256(x):
    """for s = 128, 64, .., 1: x[t] += x[t + s] for t < s"""
    x = np.array(x, dtype=np.float64)
    s = 128
    while s >= 1:
        x[:s] += x[s:2 * s]
        s //= 2
    return x[0]


def device_mean(P):
    n = P.size
    nb = (n + 255) // 256
    pad = np.zeros(nb * 256)
    pad[:n] = P
    partial = [tree256(pad[b * 256:(b + 1) * 256]) for b in range(nb)]
    x = np.zeros(256)
    for b in range(nb):                 # thread t adds the partials t, t + 256, ... in that order
        x[b % 256] += partial[b]
    return tree256(x) / n


class HostPop:
    """The population dynamics of include/mpbp_hip.h on the host; `tables[which] = (kind, values, cdf)`."""

    def __init__(self, P, beta, seed, tables):
        self.P = np.array(P, dtype=np.float64)
        self.beta, self.seed, self.tables = float(beta), int(seed), tables
        self.sweeps = self.calls = 0
        self.lib = M._lib.lib()
        self.key = (C.c_uint32 * 2)(self.seed & 0xFFFFFFFF, (self.seed >> 32) & 0xFFFFFFFF)
        self.ctr, self.out = (C.c_uint32 * 4)(), (C.c_uint32 * 4)()
        self.degrees = []               # degree of every member of the last sweep / draw

    def uniforms(self, member, slot, sweep, phase):
        self.ctr[0], self.ctr[1], self.ctr[2], self.ctr[3] = member, slot, sweep, phase
        assert self.lib.mpbp_philox4x32_10(self.ctr, self.key, self.out) == 0
        r = self.out
        return (float((r[0] >> 5) * 67108864 + (r[1] >> 6)) * 2.0 ** -53,
                float((r[2] >> 5) * 67108864 + (r[3] >> 6)) * 2.0 ** -53)

    def draw(self, which, member, slot, sweep, phase):
        kind, values, cdf = self.tables[which]
        if kind == E.DIRAC:
            return float(values[0])
        uA, uB = self.uniforms(member, slot, sweep, phase)
        if kind == E.NORMAL:
            return float(values[0]) + float(values[1]) * math.sqrt(-2.0 * math.log(1.0 - uA)) * math.cos(TWO_PI * uB)
        for j in range(len(values)):
            if cdf[j] > uA:
                return float(values[j])
        return float(values[-1])

    def field(self, which_deg, P, member, sweep, phase):
        beta, n = self.beta, P.size
        deg = int(self.draw(which_deg, member, 0, sweep, phase))
        h = self.draw(E.PH, member, 1, sweep, phase)
        self.degrees.append(deg)
        acc = 0.0
        for k in range(deg):
            uA, _ = self.uniforms(member, 2 + 2 * k, sweep, phase)
            a = min(int(math.floor(uA * float(n))), n - 1)
            J = self.draw(E.PJ, member, 3 + 2 * k, sweep, phase)
            acc += math.atanh(math.tanh(beta * P[a]) * math.tanh(beta * J))
        return (1.0 / beta) * acc + h

    def iterate(self, nsweeps):
        means = []
        for _ in range(nsweeps):
            self.sweeps += 1
            self.degrees = []
            self.P = np.array([self.field(E.PKM1, self.P, i, self.sweeps, 0) for i in range(self.P.size)])
            means.append(device_mean(self.P))
        return np.array(means)

    def magnetization(self, nsamples):
        self.calls += 1
        self.degrees = []
        return np.array([math.tanh(self.beta * self.field(E.PK, self.P, s, self.calls, 1)) for s in range(nsamples)])


def parity_tables():
    return [E.Poisson(2.5).table(), E.Poisson(2.5).table(), E.Discrete([1, -1], [0.7, 0.3]).table(),
            E.Normal(0.1, 0.5).table()]


def device_pop(P, beta, seed, tables):
    pop = M.PopDyn(P, beta=beta, seed=seed)
    for which, (kind, values, cdf) in enumerate(tables):
        pop.set_table(which, kind, values, cdf)
    return pop


# ------------------------------------------------------------------------------------------------ CPU tests
def test_exports_and_signatures():
    for name in ["equilibrium_observables", "equilibrium_magnetization", "RandomRegular", "ErdosRenyi", "CB_Pop", "Dirac",
                 "Poisson", "Discrete", "Normal", "iterate_fixedpoint"]:
        assert hasattr(M, name), name
    L = M._lib.lib()
    for name in ["mpbp_popdyn_create", "mpbp_popdyn_destroy", "mpbp_popdyn_set_distribution", "mpbp_popdyn_iterate",
                 "mpbp_popdyn_get_population", "mpbp_popdyn_set_population", "mpbp_popdyn_magnetization"]:
        assert name in M._lib.EXPORTS
        assert getattr(L, name).argtypes is not None, name
    assert "popdyn.hip" in M._lib.SOURCES
    header = open(os.path.join(ROOT, "include", "mpbp_hip.h")).read()
    assert "int mpbp_popdyn_create(mpbp_popdyn** out, int32_t device, int64_t popsize, uint64_t seed, double beta" in header


CLOSED_FORM = [  # k, J, beta, h, m, r, e
    (3, 0.8, 1.0, 0.0, 0.960701697867206, 0.942439686436436, -1.13092762372372),
    (4, 0.5, 0.7, 0.2, 0.79605740377466, 0.701681122965975, -0.860892603720907),
]


def fixed_point_numpy(k, J, beta, h, u=100.0):
    """the cavity fixed point, iterated in numpy until it stops moving"""
    f = lambda v: np.float64(k - 1) / beta * np.arctanh(np.tanh(beta * v) * np.tanh(beta * J)) + h
    u = np.float64(u)
    for _ in range(5000):
        un = f(u)
        if un == u:
            break
        u = un
    return float(u), f


@pytest.mark.parametrize("k,J,beta,h,m,r,e", CLOSED_FORM)
def test_equilibrium_observables_closed_form(k, J, beta, h, m, r, e):
    obs = M.equilibrium_observables(M.RandomRegular(k), J, beta=beta, h=h, init=100.0)
    assert obs._fields == ("m", "r", "e")
    # independently: the fixed point in numpy, the observables from it
    u, f = fixed_point_numpy(k, J, beta, h)
    assert abs(float(f(u)) - u) <= 1e-14
    t, tJ = np.tanh(beta * u), np.tanh(beta * J)
    m_np = float(np.tanh(beta * (h + (u - h) * k / (k - 1))))
    r_np = float((1 + t * t / tJ) / (1 / tJ + t * t))
    for got, ref, want in ((obs.m, m_np, m), (obs.r, r_np, r), (obs.e, -k / 2 * J * r_np - m_np * h, e)):
        assert abs(ref - want) <= 1e-12
        assert abs(got - want) <= 1e-12
    assert obs.e == -k / 2 * J * obs.r - obs.m * h


def test_equilibrium_observables_fixed_point_value():
    ustar = 1.30329212735215
    _, f = fixed_point_numpy(3, 0.8, 1.0, 0.0)
    assert abs(float(f(ustar)) - ustar) <= 1e-14
    got = M.iterate_fixedpoint(lambda u: 2 / 1.0 * math.atanh(math.tanh(u) * math.tanh(0.8)), 100.0, rtol=1e-16, atol=1e-16)
    assert abs(got - ustar) <= 1e-12


def test_equilibrium_observables_paramagnet():
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)     # a field that decays geometrically never meets a relative tolerance
        obs = M.equilibrium_observables(M.RandomRegular(3), 0.3, beta=1.0, h=0.0, init=100.0)
    assert abs(obs.m) <= 1e-14
    assert obs.e == -3 / 2 * 0.3 * obs.r - obs.m * 0.0
    with pytest.raises(TypeError):
        M.equilibrium_observables(M.ErdosRenyi(3.0), 0.3)


def test_iterate_fixedpoint_warns_when_it_does_not_converge():
    with pytest.warns(RuntimeWarning, match="did not converge"):
        M.iterate_fixedpoint(lambda u: 2 * math.atanh(math.tanh(u) * math.tanh(0.8)), 100.0, maxiter=3)


def test_distribution_tables():
    for c in (0.0, 0.5, 2.5, 20.0):
        kind, values, cdf = M.Poisson(c).table()
        assert kind == E.DISCRETE and len(values) == len(cdf) <= 256
        assert np.array_equal(values, np.arange(len(values)))
        assert np.all(np.diff(cdf) >= 0) and cdf[0] >= 0
        assert abs(cdf[-1] - 1.0) <= 2.0 ** -53
        # against the pmf evaluated term by term and summed exactly
        pm = lambda k: math.exp(-c + k * math.log(c) - math.lgamma(k + 1)) if c > 0 else float(k == 0)
        K = len(values) - 1
        want = np.array([math.fsum(pm(j) for j in range(k + 1)) for k in range(K)])
        assert np.abs(cdf[:-1] - want).max(initial=0.0) <= 1e-13
        # K is the first k whose upper tail is below 2^-53
        tail = lambda k: math.fsum(pm(j) for j in range(k + 1, k + 100))
        assert tail(K) < 2.0 ** -53 and (K == 0 or tail(K - 1) >= 2.0 ** -53)
    with pytest.raises(ValueError):
        M.Poisson(200).table()
    with pytest.raises(ValueError):
        M.Discrete([1, -1], [0.7, 0.2])
    kind, values, cdf = M.Discrete([1, -1], [0.7, 0.3]).table()
    assert kind == E.DISCRETE and list(values) == [1.0, -1.0] and list(cdf) == [0.7, 1.0]
    assert M.Dirac(2).table()[0] == E.DIRAC and M.Normal(0.1, 0.5).table()[0] == E.NORMAL
    with pytest.raises(TypeError):
        M.equilibrium_magnetization(M.RandomRegular(3), pJ=0.8)
    with pytest.raises(TypeError):
        M.equilibrium_magnetization("poisson", M.Dirac(3))


def test_host_restatement_is_self_consistent():
    """the draws of a sweep depend on the sweep's number, not on how the calls are split: 4 sweeps = 2 + 2"""
    P0 = np.random.default_rng(3).standard_normal(40)
    a, b = HostPop(P0, 0.7, 11, parity_tables()), HostPop(P0, 0.7, 11, parity_tables())
    ma = a.iterate(4)
    mb = np.concatenate([b.iterate(2), b.iterate(2)])
    assert np.array_equal(a.P, b.P) and np.array_equal(ma, mb)
    assert not np.array_equal(a.P, HostPop(P0, 0.7, 12, parity_tables()).iterate(4))
    assert np.array_equal(a.magnetization(7), b.magnetization(7))
    # the tree of the mean against an exact sum
    x = np.random.default_rng(0).standard_normal(1000)
    assert abs(device_mean(x) - math.fsum(x) / 1000) <= 1e-15


# ------------------------------------------------------------------------------------------------ GPU tests
@pytest.mark.gpu
@pytest.mark.parametrize("popsize", [1, 255, 256, 257, 1000])
def test_popdyn_matches_the_host_restatement(popsize):
    """every member after each of 3 sweeps, the per-sweep means and 300 magnetisation samples, to 1e-12 absolute"""
    beta, seed, tabs = 0.7, 2024, parity_tables()
    P0 = np.random.default_rng(popsize).standard_normal(popsize)
    host, dev = HostPop(P0, beta, seed, tabs), device_pop(P0, beta, seed, tabs)
    gap, zero_degree = 0.0, []
    for _ in range(3):
        hm, dm = host.iterate(1), dev.iterate(1)
        Pd = dev.get_population()
        gap = max(gap, np.abs(Pd - host.P).max(), np.abs(dm - hm).max())
        zero_degree.append([i for i, deg in enumerate(host.degrees) if deg == 0])
    gap = max(gap, np.abs(dev.magnetization(300) - host.magnetization(300)).max())
    print(f"popsize {popsize}: max |device - host| = {gap:.3e}, {sum(map(len, zero_degree))} members of degree 0")
    assert popsize < 255 or zero_degree[0]
    assert gap <= 1e-12
    # a member of degree 0 equals its field bit for bit: the same sweep with a field the host restates without libm
    # (slot 0 does not depend on ph, so the degrees are those of the first sweep above)
    ph = E.Discrete([0.3, -0.2, 1.7], [0.5, 0.3, 0.2]).table()
    host0, dev0 = HostPop(P0, beta, seed, tabs[:3] + [ph]), device_pop(P0, beta, seed, tabs[:3] + [ph])
    dev0.iterate(1)
    Pd = dev0.get_population()
    for i in zero_degree[0]:
        assert Pd[i] == host0.draw(E.PH, i, 1, 1, 0)


@pytest.mark.gpu
def test_popdyn_is_reproducible():
    tabs = parity_tables()
    P0 = np.random.default_rng(5).standard_normal(700)
    a, b, c = device_pop(P0, 0.7, 9, tabs), device_pop(P0, 0.7, 9, tabs), device_pop(P0, 0.7, 10, tabs)
    ma = a.iterate(4)
    mb = np.concatenate([b.iterate(1) for _ in range(4)])
    Pa = a.get_population()
    assert np.array_equal(ma, mb) and np.array_equal(Pa, b.get_population())
    c.iterate(4)
    assert not np.array_equal(Pa, c.get_population())
    a.set_population(Pa)
    assert np.array_equal(a.get_population(), Pa)
    assert np.array_equal(a.magnetization(100), b.magnetization(100))
    assert np.array_equal(a.iterate(2), b.iterate(2)) and np.array_equal(a.get_population(), b.get_population())


@pytest.mark.gpu
@pytest.mark.parametrize("h,m_exact", [(0.0, 0.960701697867206), (0.1, 0.974503691296974)])
def test_reference_testcase_random_regular(h, m_exact):
    """test/equilibrium.jl of the reference: population dynamics on RandomRegular(3) against the closed form"""
    m_eq = M.equilibrium_observables(M.RandomRegular(3), 0.8, beta=1.0, h=h, init=100.0).m
    assert abs(m_eq - m_exact) <= 1e-12
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)     # tol = 1e-15 is at the rounding level of the mean
        m_avg, m_std = M.equilibrium_magnetization(M.RandomRegular(3), pJ=M.Dirac(0.8), ph=M.Dirac(h), beta=1.0,
                                                   popsize=10 ** 5, tol=1e-15, maxiter=100)
    print(f"h = {h}: m_avg = {m_avg!r}, closed form {m_eq!r}, m_std = {m_std:.3e}")
    assert abs(m_avg - m_eq) <= 1.5e-8 * max(abs(m_avg), abs(m_eq))
    assert m_std <= 1e-8


@pytest.mark.gpu
def test_paramagnet_contracts_to_zero():
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        m_avg, m_std = M.equilibrium_magnetization(M.ErdosRenyi(2.0), pJ=M.Dirac(1.0), beta=0.3, ph=M.Dirac(0.0),
                                                   popsize=4096, maxiter=100, tol=0.0)
    print(f"paramagnet: m_avg = {m_avg:.3e}")
    assert m_avg <= 1e-12


@pytest.mark.gpu
def test_cb_pop():
    # positive fields: a sum of 1000 positive numbers has a relative error of a few 2^-53 in any tree order
    P0 = np.abs(np.random.default_rng(1).standard_normal(1000)) + 0.5
    kw = dict(pJ=M.Dirac(0.8), beta=1.0, popsize=1000, P=P0, tol=0.0, nsamples=10, seed=4)
    seen, calls = [], []

    def median(P):
        seen.append(P.copy())
        return float(np.median(P))

    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        cb1, cbf, cb5 = M.CB_Pop(), M.CB_Pop(f=median), M.CB_Pop(f=lambda P: calls.append(P.copy()) or float(np.median(P)))
        M.equilibrium_magnetization(M.RandomRegular(3), maxiter=10, cb=cb1, **kw)
        M.equilibrium_magnetization(M.RandomRegular(3), maxiter=10, cb=cbf, **kw)
        M.equilibrium_magnetization(M.RandomRegular(3), maxiter=10, cb=cb5, check_every=5, **kw)
    assert cb1.m[0] == math.inf and len(cb1.m) == 11 and len(cb1.Δs) == 10
    assert len(cbf.m) == 11 and len(cbf.Δs) == 10 and len(seen) == 10 and seen[0].shape == (1000,)
    for i in range(10):
        ref = float(np.mean(seen[i]))
        assert abs(cb1.m[i + 1] - ref) <= 1e-13 * abs(ref)
        assert cbf.m[i + 1] == float(np.median(seen[i]))
    assert cb1.Δs[0] == math.inf and cb1.Δs[3] == abs(cb1.m[4] - cb1.m[3])
    assert len(cb5.m) == 3 and len(cb5.Δs) == 2 and len(calls) == 2
    assert np.array_equal(calls[0], seen[4]) and np.array_equal(calls[1], seen[9])


@pytest.mark.gpu
def test_refusals_leave_the_handle_usable():
    tabs = parity_tables()
    P0 = np.random.default_rng(8).standard_normal(300)

    def refused(fn, *a, **k):
        with pytest.raises(M.MPBPError) as ei:
            fn(*a, **k)
        assert ei.value.code == -1, ei.value

    pop = M.PopDyn(P0, beta=0.7, seed=6)
    refused(M.PopDyn, np.zeros(0))                                  # popsize = 0
    refused(M.PopDyn, P0, beta=0.0)
    refused(M.PopDyn, P0, beta=float("inf"))
    refused(pop.iterate, 1)                                         # no distribution set yet
    for which, (kind, values, cdf) in enumerate(tabs):
        pop.set_table(which, kind, values, cdf)
    refused(pop.set_table, E.PJ, E.DISCRETE, [1.0, -1.0], [0.7, 0.3])     # non-monotone cdf: the table before it stays
    refused(pop.set_table, E.PKM1, E.NORMAL, [2.0, 1.0])                  # a degree is DIRAC or DISCRETE
    refused(pop.set_table, E.PK, E.DISCRETE, np.zeros(257), np.ones(257))
    refused(pop.iterate, 0)
    refused(pop.magnetization, 0)
    host = HostPop(P0, 0.7, 6, tabs)
    assert np.abs(pop.iterate(2) - host.iterate(2)).max() <= 1e-12
    assert np.abs(pop.get_population() - host.P).max() <= 1e-12
    assert np.abs(pop.magnetization(50) - host.magnetization(50)).max() <= 1e-12
