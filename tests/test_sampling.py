"""SoftMargin sampler (reference src/sampling.jl; C ABI mpbp_sampler_* in include/mpbp_hip.h).

The host restatement below - Philox4x32-10 in numpy, the RecursiveBPFactor functor folded from the same dense tables in
the reference's order (src/recursive_bp_factor.jl:33-45), `sample_noalloc` (src/utils.jl:8-19) and the log-weight of
src/sampling.jl:46-53 - reproduces every device draw; the distribution tests check the sampler against brute-force
enumeration (oracle/exact.py) and against MPBP beliefs on a tree."""
import ctypes as C
import os

import numpy as np
import pytest

import mpbp_amd as M
from oracle import factors as OF
from oracle import mpbp as O
from oracle.exact import exact_autocorrelations, exact_marginals, exact_pair_marginals, exact_prob

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MASK = np.uint64(0xFFFFFFFF)


# ------------------------------------------------------------------------------------------------ host restatement
def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Random123 Philox4x32-10 on numpy arrays of 32-bit words (held in uint64)."""
    c0, c1, c2, c3 = (np.asarray(v, dtype=np.uint64) & MASK for v in (c0, c1, c2, c3))
    k0, k1 = np.uint64(k0) & MASK, np.uint64(k1) & MASK
    for _ in range(10):
        p0 = np.uint64(0xD2511F53) * c0
        p1 = np.uint64(0xCD9E8D57) * c2
        c0, c1, c2, c3 = ((p1 >> np.uint64(32)) ^ c1 ^ k0) & MASK, p1 & MASK, ((p0 >> np.uint64(32)) ^ c3 ^ k1) & MASK, p0 & MASK
        k0 = (k0 + np.uint64(0x9E3779B9)) & MASK
        k1 = (k1 + np.uint64(0xBB67AE85)) & MASK
    return c0, c1, c2, c3


def uniforms(seed, samples, L, N):
    """u[s, t, i] of global sample index samples[s]: counter (index lo, hi, t, node), key = seed."""
    s = np.asarray(samples, dtype=np.uint64)[:, None, None]
    t = np.arange(L, dtype=np.uint64)[None, :, None]
    i = np.arange(N, dtype=np.uint64)[None, None, :]
    shp = (s.shape[0], L, N)
    r0, r1, _, _ = philox4x32_10(np.broadcast_to(s & MASK, shp), np.broadcast_to(s >> np.uint64(32), shp),
                                 np.broadcast_to(t, shp), np.broadcast_to(i, shp), seed & 0xFFFFFFFF, seed >> 32)
    return ((r0 >> np.uint64(5)).astype(np.float64) * 67108864.0 + (r1 >> np.uint64(6)).astype(np.float64)) * 2.0 ** -53


class HostSampler:
    """Restatement of the device sampler: same tables, same arithmetic order, same uniforms."""

    def __init__(self, bp):
        self.bp, self.q, self.T, self.N = bp, bp.q, bp.T, bp.g.nv()
        self.nbrs = [[int(v) for v in bp.g.neighbors(i)] for i in range(self.N)]
        self._tabs = {}

    def _tab(self, wt, deg):
        k = (id(wt), deg)
        if k not in self._tabs:
            if isinstance(wt, M.RecursiveBPFactor):
                ny, py, pxy, pyy, py0 = wt.tables(deg, self.q)
                off, o = {}, 0
                for d1 in range(deg + 1):
                    for d2 in range(deg - d1 + 1):
                        off[(d1, d2)] = o
                        o += int(ny[d1 + d2] * ny[d1] * ny[d2]) * self.q
                self._tabs[k] = ("rec", [int(v) for v in ny], py.tolist(), pxy.tolist(), pyy.tolist(), py0.tolist(), off)
            else:
                self._tabs[k] = ("gen", wt.generic_table(deg, self.q).tolist())
        return self._tabs[k]

    def probs(self, i, t, x, xs):
        """w[i][t](x', xs, x) for x' over the node's states (x, xs 0-based)."""
        q, qi = self.q, int(self.bp.qnode[i])
        deg = len(xs)
        tb = self._tab(self.bp.w[i][t], deg)
        if tb[0] == "gen":
            col = 0
            for xk in reversed(xs):
                col = col * q + xk
            col = (col * q + x) * q
            return [tb[1][col + xx] for xx in range(qi)]
        _, ny, py, pxy, pyy, py0, off = tb
        ny1 = ny[1] if deg > 0 else 1
        P = [py0[y + ny[0] * x] for y in range(ny[0])]
        for k in range(1, deg + 1):
            xk, nyk, ln, b = xs[k - 1], ny[k], len(P), off[(1, k - 1)]
            bxy = (k - 1) * ny1 * q * q + ny1 * (xk + q * x)
            Pn = []
            for y in range(nyk):
                acc = 0.0
                for y2 in range(ln):
                    for y1 in range(ny1):
                        acc += pyy[b + y + nyk * (y1 + ny1 * (y2 + ln * x))] * pxy[bxy + y1] * P[y2]
                Pn.append(acc)
            P = Pn
        out = []
        for xx in range(qi):
            p = 0.0
            for y in range(len(P)):
                p += P[y] * py[xx + q * (x + q * y)]
            out.append(p)
        return out

    @staticmethod
    def draw(ps, u):
        """sample_noalloc; also reports whether u lies within 1e-12 of a cumulative boundary"""
        cw, pick, last, near = 0.0, -1, 0, False
        for xx, p in enumerate(ps):
            if p > 0:
                last = xx
            cw += p
            near = near or abs(cw - u) < 1e-12
            if cw > u:
                pick = xx
                break
        return (pick if pick >= 0 else last), near

    def trajectories(self, seed, samples):
        """X[s] 0-based [T+1, N], logw[s], near-boundary flags"""
        bp, N, L, q = self.bp, self.N, self.T + 1, self.q
        U = uniforms(seed, samples, L, N)
        X = np.zeros((len(samples), L, N), dtype=np.int64)
        near = np.zeros(len(samples), dtype=bool)
        for s in range(len(samples)):
            for i in range(N):
                qi = int(bp.qnode[i])
                z = 0.0
                for x in range(qi):
                    z += bp.phi[x, 0, i]
                X[s, 0, i], nb = self.draw([bp.phi[x, 0, i] / z for x in range(qi)], U[s, 0, i])
                near[s] |= nb
            for t in range(L - 1):
                for i in range(N):
                    ps = self.probs(i, t, int(X[s, t, i]), [int(X[s, t, j]) for j in self.nbrs[i]])
                    X[s, t + 1, i], nb = self.draw(ps, U[s, t + 1, i])
                    near[s] |= nb
        return X, np.array([self.logw(x) for x in X]), near

    def logw(self, x):
        bp = self.bp
        with np.errstate(divide="ignore"):
            lw = 0.0
            for t in range(1, self.T + 1):
                for i in range(self.N):
                    lw += np.log(bp.phi[x[t, i], t, i])
            for t in range(self.T + 1):
                for (i, j, e) in bp.g.edges():
                    lw += 0.5 * np.log(bp.psi[x[t, i], x[t, j], t, e])
        return lw


def _draw_raw(sms, n):
    """n samples through the C entry point, trajectories returned as [n, T+1, N] 0-based (no per-sample host objects)"""
    bp = sms.bp
    X = np.zeros((n, bp.T + 1, bp.g.nv()), dtype=np.uint8)
    lw = np.zeros(n)
    sms._check(sms._L.mpbp_sample(sms._h, n, X.ctypes.data_as(C.POINTER(C.c_uint8)),
                                  lw.ctypes.data_as(C.POINTER(C.c_double))))
    return X, lw


# ------------------------------------------------------------------------------------------------ models
STAR = np.array([[0, 1, 1, 1], [1, 0, 0, 0], [1, 0, 0, 0], [1, 0, 0, 0]])


def _star_sis(T=2, observe=False, psi=False, seed=111):
    """reference test/sampling.jl:1-20: SIS(g, λ=0.5, ρ=0.2, T; γ=0.5, α=0.1) on the star of 4"""
    lam, rho, gam, alpha = 0.5, 0.2, 0.5, 0.1
    phi = [[np.array([1 - gam, gam]) if t == 0 else np.ones(2) for t in range(T + 1)] for _ in range(4)]
    g = M.IndexedBiDiGraph(STAR)
    ps = None
    if psi:
        rng = np.random.default_rng(seed)
        base = {}
        ps = []
        for (i, j, _) in g.edges():
            key = (min(i, j), max(i, j))
            if key not in base:
                base[key] = [rng.random((2, 2)) + 0.2 for _ in range(T + 1)]
            ps.append([m if i < j else m.T.copy() for m in base[key]])
    bp = M.mpbp(g, [[M.SISFactor(lam, rho, alpha)] * (T + 1)] * 4, 2, T, phi=phi, psi=ps, max_bond=16)
    if observe:
        M.draw_node_observations(bp, 4, last_time=True, softinf=1e2, rng=np.random.default_rng(seed))
    return bp


def _oracle_of(bp, factors):
    """the oracle model of a device MPBP (same graph, factors, current phi and psi) for exact enumeration"""
    A = np.zeros((bp.g.nv(), bp.g.nv()), dtype=int)
    for (i, j, _) in bp.g.edges():
        A[i, j] = 1
    og = O.IndexedBiDiGraph(A)
    assert [tuple(int(v) for v in e) for e in og.edges()] == bp.g.edges()
    qs = [int(v) for v in bp.qnode]
    phi = [[bp.phi[:qs[i], t, i].copy() for t in range(bp.T + 1)] for i in range(bp.g.nv())]
    psi = [[bp.psi[:qs[i], :qs[j], t, e].copy() for t in range(bp.T + 1)] for (i, j, e) in bp.g.edges()]
    return O.mpbp(og, factors, qs, bp.T, phi=phi, psi=psi)


def _glauber_tree():
    T = 2
    J = np.array([[0, 1, 0, 0, 0], [1, 0, 1, 1, 0], [0, 1, 0, 0, 0], [0, 1, 0, 0, 0], [0, 0, 0, 0, 0]], float)
    h = np.random.default_rng(111).standard_normal(5)
    phi = [[np.array([0.75, 0.25]) if t == 0 else np.ones(2) for t in range(T + 1)] for _ in range(5)]
    phi[1][2] = np.array([0.2, 0.8])
    phi[3][1] = np.array([0.9, 0.1])
    bp = M.Glauber(M.Ising(J, h, 1.0), T, phi=phi).mpbp(max_bond=16)
    assert max(bp.w[1][0].nstates(l) for l in range(4)) > 2
    return bp


def _sirs_tree():
    T = 3
    A = np.array([[0, 1, 1], [1, 0, 0], [1, 0, 0]])
    phi = [[np.array([0.5, 0.5, 0.0]) if t == 0 else np.ones(3) for t in range(T + 1)] for _ in range(3)]
    phi[2][2] = np.array([0.1, 0.3, 0.6])
    return M.mpbp(M.IndexedBiDiGraph(A), [[M.SIRSFactor(0.4, 0.4, 0.3, 0.05)] * (T + 1)] * 3, 3, T, phi=phi, max_bond=27)


def _hetero_tree():
    T = 2
    A = np.array([[0, 1, 1, 0], [1, 0, 0, 1], [1, 0, 0, 0], [0, 1, 0, 0]])
    qs = [2, 3, 2, 3]
    rng = np.random.default_rng(0)
    phi = [[rng.random(q) + 0.1 for _ in range(T + 1)] for q in qs]
    w = [[M.SISFactor(0.3, 0.2)] * (T + 1) if q == 2 else [M.SIRSFactor(0.3, 0.2, 0.1)] * (T + 1) for q in qs]
    return M.mpbp(M.IndexedBiDiGraph(A), w, qs, T, phi=phi, max_bond=16)


def _generic_star():
    T = 3
    w = [[M.GenericFactor(M.SISFactor(0.5, 0.2, 0.1))] * (T + 1), [M.SISFactor(0.5, 0.2, 0.1)] * (T + 1),
         [M.GenericFactor(M.SISFactor(0.4, 0.3))] * (T + 1), [M.SISFactor(0.6, 0.1)] * (T + 1)]
    phi = [[np.array([0.5, 0.5]) if t == 0 else np.array([0.3, 0.7]) for t in range(T + 1)] for _ in range(4)]
    return M.mpbp(M.IndexedBiDiGraph(STAR), w, 2, T, phi=phi, max_bond=4)


def _time_dependent_star():
    T = 4
    w = [[M.SISFactor(0.2 + 0.15 * t, 0.1 + 0.05 * t, 0.05) for t in range(T + 1)] for _ in range(4)]
    phi = [[np.array([0.6, 0.4]) if t == 0 else np.array([1.0, 0.5 + 0.1 * t]) for t in range(T + 1)] for _ in range(4)]
    return M.mpbp(M.IndexedBiDiGraph(STAR), w, 2, T, phi=phi, max_bond=16)


def _karate_glauber():
    A = np.loadtxt(os.path.join(ROOT, "tests", "golden", "karate.txt"))
    T = 3
    N = A.shape[0]
    h = np.random.default_rng(3).standard_normal(N) * 0.3
    phi = [[np.array([0.5, 0.5]) if t == 0 else np.array([0.6, 0.4]) for t in range(T + 1)] for _ in range(N)]
    bp = M.Glauber(M.Ising(0.3 * (A != 0), h, 1.0), T, phi=phi).mpbp(max_bond=4)
    assert max(bp.g.degree(i) for i in range(N)) == 17
    return bp


# ------------------------------------------------------------------------------------------------ CPU
KAT = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
       ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
       ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
        (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]


@pytest.mark.parametrize("ctr,key,want", KAT)
def test_philox_known_answers(ctr, key, want):
    """Random123's known-answer vectors for Philox4x32-10: the numpy restatement and the library's own block function."""
    got = philox4x32_10(*ctr, *key)
    assert tuple(int(v) for v in got) == want
    L = M._lib.lib()
    out = (C.c_uint32 * 4)()
    assert L.mpbp_philox4x32_10((C.c_uint32 * 4)(*ctr), (C.c_uint32 * 2)(*key), out) == 0
    assert tuple(out) == want


def test_sampler_names_exported_with_ctypes_signatures():
    for name in ("SoftMarginSampler", "sample", "onesample", "marginals", "pair_marginals", "means", "autocorrelations",
                 "autocovariances", "effective_sample_size", "mean_with_uncertainty", "draw_node_observations"):
        assert hasattr(M, name), name
    L = M._lib.lib()
    for name in ("mpbp_sampler_create", "mpbp_sampler_destroy", "mpbp_sample", "mpbp_sampler_marginals",
                 "mpbp_sampler_pair_marginals", "mpbp_sampler_twovar_marginals", "mpbp_sampler_counts", "mpbp_philox4x32_10"):
        assert name in M._lib.EXPORTS
        assert getattr(L, name).argtypes is not None, name
    header = open(os.path.join(ROOT, "include", "mpbp_hip.h")).read()
    assert "int mpbp_sampler_create(mpbp_sampler** out, mpbp_ctx* ctx, uint64_t seed, const int32_t* corr_nodes" in header
    assert len(L.mpbp_sampler_create.argtypes) == 6 and L.mpbp_sampler_create.argtypes[2] is C.c_uint64
    assert len(L.mpbp_sample.argtypes) == 4 and L.mpbp_sample.argtypes[1] is C.c_int64


def test_mean_with_uncertainty():
    v, e = M.mean_with_uncertainty([1.0, 2.0, 3.0], [0.3, 0.4, 0.0])
    assert v == pytest.approx(2.0) and e == pytest.approx(0.5 / 3)


# ------------------------------------------------------------------------------------------------ GPU
CASES = {"star_sis_observed_psi": lambda: _star_sis(T=2, observe=True, psi=True), "glauber_tree": _glauber_tree,
         "sirs_q3": _sirs_tree, "heterogeneous_sis_sirs": _hetero_tree, "generic_factor": _generic_star,
         "time_dependent": _time_dependent_star, "karate_hub_deg17": _karate_glauber}


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(CASES))
def test_trajectories_match_host_restatement(case):
    bp = CASES[case]()
    n = 60 if case == "karate_hub_deg17" else 400
    seed = 0x1234_5678_9ABC + len(case)
    sms = M.sample(bp, n, seed=seed, keep_samples=True)
    X = np.array([x.T - 1 for x in sms.X])            # [s][t][i] 0-based
    hX, hlw, near = HostSampler(bp).trajectories(seed, np.arange(n))
    assert near.sum() == 0 or near.sum() < n // 100, f"{near.sum()} draws near a boundary"
    ok = ~near
    assert np.array_equal(X[ok], hX[ok])
    np.testing.assert_allclose(sms.logw[ok], hlw[ok], rtol=0, atol=1e-12)
    assert all(x.min() >= 1 and all(x[i].max() <= bp.qnode[i] for i in range(bp.g.nv())) for x in sms.X)


@pytest.mark.gpu
def test_decomposition_independence():
    bp = _star_sis(T=3, observe=True, psi=True)
    a = M.sample(bp, 1000, seed=7, keep_samples=True, autocorr_sites=[0, 2])
    b = M.sample(bp, 300, seed=7, keep_samples=True, autocorr_sites=[0, 2])
    M.sample(b, 700)
    c = M.SoftMarginSampler(bp, seed=7, keep_samples=True, autocorr_sites=[0, 2])
    for k in (333, 333, 334):
        M.sample(c, k)
    for o in (b, c):
        assert o.nsamples == 1000
        assert all(np.array_equal(x, y) for x, y in zip(a.X, o.X)) and len(o.X) == 1000
        assert np.array_equal(a.logw, o.logw)
        for fa, fo in ((M.marginals(a)[0], M.marginals(o)[0]), (M.pair_marginals(a)[0], M.pair_marginals(o)[0])):
            assert max(np.abs(np.array(x) - np.array(y)).max() for x, y in zip(fa, fo)) < 1e-12
        ra, ro = M.autocorrelations(lambda x, i: x - 1, a)[0], M.autocorrelations(lambda x, i: x - 1, o)[0]
        assert max(np.abs(x - y).max() for x, y in zip(ra, ro)) < 1e-12
    d = M.sample(bp, 1000, seed=8, keep_samples=True)
    assert not np.array_equal(a.logw, d.logw) or not all(np.array_equal(x, y) for x, y in zip(a.X, d.X))


def _within(val, ref, sig, k=5.0):
    val, ref, sig = np.asarray(val), np.asarray(ref), np.asarray(sig)
    dev = np.abs(val - ref)
    return bool(np.all(dev <= k * sig + 1e-12)), float(np.max(dev / (sig + 1e-300)))


@pytest.mark.gpu
def test_prior_distribution_matches_enumeration():
    T = 2
    bp = _star_sis(T=T)
    obp = _oracle_of(bp, [[OF.SISFactor(0.5, 0.2, 0.1)] * (T + 1)] * 4)
    with np.errstate(divide="ignore"):
        p, _ = exact_prob(obp)
    n = 4 * 10 ** 6
    sms = M.SoftMarginSampler(bp, seed=2024, autocorr_sites=[0, 1, 2, 3])
    X, lw = _draw_raw(sms, n)
    assert np.all(lw == 0.0)                             # free dynamics: every weight is one
    assert M.effective_sample_size(sms) == pytest.approx(n, rel=1e-12)
    # node, pair, two-time marginals within 5 sigma of the exact ones
    m, _ = M.marginals(sms)
    em = exact_marginals(obp, p)
    for i in range(4):
        for t in range(T + 1):
            pe = np.asarray(em[i][t])
            ok, z = _within(m[i][t], pe, np.sqrt(pe * (1 - pe) / n))
            assert ok, (i, t, z)
    pm, _ = M.pair_marginals(sms)
    epm = exact_pair_marginals(obp, p)
    for e in range(bp.g.ne()):
        for t in range(T + 1):
            pe = np.asarray(epm[e][t])
            ok, z = _within(pm[e][t], pe, np.sqrt(pe * (1 - pe) / n))
            assert ok, (e, t, z)
    f = lambda x, i: float(x == 2)
    r, _ = M.autocorrelations(f, sms)
    er = exact_autocorrelations(f, obp, p)
    for i in range(4):
        for t in range(T + 1):
            for u in range(t + 1, T + 1):
                pe = er[i][t, u]
                ok, z = _within(r[i][t, u], pe, np.sqrt(pe * (1 - pe) / n))
                assert ok, (i, t, u, z)
    # chi^2 of the histogram of whole trajectories against exact_prob (axes node-major, time inside)
    idx = np.zeros(n, dtype=np.int64)
    for i in range(4):
        for t in range(T + 1):
            idx = idx * 2 + X[:, t, i]
    counts = np.bincount(idx, minlength=p.size)
    expct = n * p.ravel()
    assert counts[expct == 0].sum() == 0
    big = expct >= 5
    obs = np.append(counts[big], counts[~big].sum())
    exp_ = np.append(expct[big], expct[~big].sum())
    if exp_[-1] == 0:
        obs, exp_ = obs[:-1], exp_[:-1]
    chi2 = float(np.sum((obs - exp_) ** 2 / exp_))
    dof = obs.size - 1
    assert chi2 < dof + 6 * np.sqrt(2 * dof), (chi2, dof)


@pytest.mark.gpu
def test_posterior_matches_enumeration():
    T = 2
    bp = _star_sis(T=T)
    phi0 = bp.phi.copy()
    X, observed = M.draw_node_observations(bp, 4, last_time=True, softinf=1e2, rng=np.random.default_rng(111))
    assert X.shape == (4, T + 1) and X.min() >= 1 and X.max() <= 2
    assert observed == sorted(observed) and [t for (_, t) in observed] == [T] * 4
    changed = {(i, t) for i in range(4) for t in range(T + 1) if not np.array_equal(bp.phi[:, t, i], phi0[:, t, i])}
    assert changed == set(observed)
    for (i, t) in observed:
        want = np.where(np.arange(2) == X[i, t] - 1, 1 / (1 + 1e-2), 1 / (1 + 1e2))
        np.testing.assert_allclose(bp.phi[:, t, i], want, rtol=1e-15)
    assert not M.is_free_dynamics(bp)
    obp = _oracle_of(bp, [[OF.SISFactor(0.5, 0.2, 0.1)] * (T + 1)] * 4)
    with np.errstate(divide="ignore"):
        p, _ = exact_prob(obp)
    n = 2 * 10 ** 6
    sms = M.sample(bp, n, seed=99, autocorr_sites=[0])
    neff = M.effective_sample_size(sms)
    assert 0.01 * n < neff < n
    m, _ = M.marginals(sms)
    em = exact_marginals(obp, p)
    for i in range(4):
        for t in range(T + 1):
            pe = np.asarray(em[i][t])
            ok, z = _within(m[i][t], pe, np.sqrt(pe * (1 - pe) / neff))
            assert ok, (i, t, z)
    pm, _ = M.pair_marginals(sms)
    epm = exact_pair_marginals(obp, p)
    for e in range(bp.g.ne()):
        for t in range(T + 1):
            pe = np.asarray(epm[e][t])
            ok, z = _within(pm[e][t], pe, np.sqrt(pe * (1 - pe) / neff))
            assert ok, (e, t, z)


@pytest.mark.gpu
def test_sampled_marginals_match_mpbp_on_a_tree():
    T = 3
    bp = _star_sis(T=T, observe=True, psi=True, seed=5)
    M.iterate(bp, maxiter=10, svd_trunc=M.TruncBond(16), tol=1e-14)
    n = 10 ** 6
    sms = M.sample(bp, n, seed=11)
    neff = M.effective_sample_size(sms)
    b = M.beliefs(bp)
    m, _ = M.marginals(sms)
    for i in range(4):
        for t in range(T + 1):
            pe = np.asarray(b[i][t])
            ok, z = _within(m[i][t], pe, np.sqrt(pe * (1 - pe) / neff))
            assert ok, (i, t, z)
    pb, _ = M.pair_beliefs(bp)
    pm, _ = M.pair_marginals(sms)
    for e in range(bp.g.ne()):
        for t in range(T + 1):
            pe = np.asarray(pb[e][t])
            ok, z = _within(pm[e][t], pe, np.sqrt(pe * (1 - pe) / neff))
            assert ok, (e, t, z)
    mv, me = M.means(lambda x, i: x - 1, sms)
    assert all(np.all((0 <= v) & (v <= 1)) and np.all(e >= 0) for v, e in zip(mv, me))


@pytest.mark.gpu
def test_weight_identity_with_logprob():
    bp = _star_sis(T=3, observe=True, psi=True, seed=17)
    sms = M.sample(bp, 200, seed=3, keep_samples=True)
    N, T = 4, 3
    nbrs = [[int(v) for v in bp.g.neighbors(i)] for i in range(N)]
    assert np.all(bp.phi[:2, 0, :].sum(axis=0) == 1.0)     # phi^0 normalised: logprob's phi^0 term is log p^0
    for x, lw in zip(sms.X, sms.logw):
        lp = M.logprob(bp, x)
        assert np.isfinite(lp)                               # every kept sample has nonzero prior probability
        lp0 = sum(np.log(bp.phi[x[i, 0] - 1, 0, i] / bp.phi[:2, 0, i].sum()) for i in range(N))
        lt = sum(np.log(bp.w[i][t](int(x[i, t + 1]), [int(x[j, t]) for j in nbrs[i]], int(x[i, t])))
                 for t in range(T) for i in range(N))
        assert abs(lw - (lp - lp0 - lt)) < 1e-10


@pytest.mark.gpu
def test_full_size_config1():
    import networkx as nx
    N, T = 1024, 50
    A = nx.to_numpy_array(nx.random_regular_graph(3, N, seed=0), nodelist=range(N))
    phi = [[np.array([0.9, 0.1]) if t == 0 else np.ones(2) for t in range(T + 1)] for _ in range(N)]
    bp = M.mpbp(M.IndexedBiDiGraph(A), [[M.SISFactor(0.1, 0.05)] * (T + 1)] * N, 2, T, phi=phi, max_bond=4)
    sms = M.sample(bp, 10 ** 5, seed=5, autocorr_sites=list(range(16)))
    m, _ = M.marginals(sms)
    arr = np.array(m)
    assert np.all(np.isfinite(arr)) and np.abs(arr.sum(axis=2) - 1).max() < 1e-12
    pm, _ = M.pair_marginals(sms)
    assert np.abs(np.array(pm).sum(axis=(2, 3)) - 1).max() < 1e-12
    few = M.sample(bp, 4, seed=5, keep_samples=True)
    hX, hlw, near = HostSampler(bp).trajectories(5, np.arange(4))
    assert not near.any()
    assert np.array_equal(np.array([x.T - 1 for x in few.X]), hX)
    np.testing.assert_allclose(few.logw, hlw, rtol=0, atol=1e-12)


@pytest.mark.gpu
def test_sampler_error_paths_do_not_abort():
    bp = _star_sis(T=2)
    sms = M.SoftMarginSampler(bp)
    with pytest.raises(M.MPBPError):
        M.marginals(sms)                                     # nothing drawn yet
    with pytest.raises(M.MPBPError) as ei:
        M.sample(sms, 0)
    assert ei.value.code == -1
    with pytest.raises(M.MPBPError):
        M.sample(sms, -3)
    with pytest.raises(ValueError):
        M.autocorrelations(lambda x, i: x, M.sample(bp, 10))
    s2 = M.sample(bp, 10, autocorr_sites=[1])
    with pytest.raises(ValueError):
        M.autocorrelations(lambda x, i: x, s2, sites=[2])
    # aliased graphs: refused by the mirror and by the library itself
    ibp = M.mpbp_infinite_graph(3, [M.SISFactor(0.1, 0.2)] * 3, 2)
    with pytest.raises(M.MPBPError) as ei:
        M.sample(ibp, 10)
    assert ei.value.code == -4
    h = C.c_void_p()
    assert ibp._L.mpbp_sampler_create(C.byref(h), ibp._h, 0, None, 0, 0) == -4
    with pytest.raises(M.MPBPError):
        M.sample(M.mpbp_infinite_bipartite_graph((2, 3), [[M.SISFactor(0.1, 0.2)] * 3] * 2, (2, 2)), 10)
    # every trajectory excluded by an observation: marginals report it
    bp.phi[:, 1, 0] = 0.0
    M._lib.check(bp._L.mpbp_set_phi(bp._h, bp.phi.ravel(order="F").ctypes.data_as(C.POINTER(C.c_double))), bp._h)
    z = M.sample(bp, 100)
    assert np.all(np.isneginf(z.logw))
    with pytest.raises(M.MPBPError) as ei:
        M.marginals(z)
    assert ei.value.code == -1 and "zero" in str(ei.value)
