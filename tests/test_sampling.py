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


def _star_sis(T=2, observe=False, psi=False, seed=111, host=False):
    """reference test/sampling.jl:1-20: SIS(g, λ=0.5, ρ=0.2, T; γ=0.5, α=0.1) on the star of 4 (host: the same model as a
    _HostModel, built and observed without a device)"""
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
    if host:
        hm = _HostModel(g, [[M.SISFactor(lam, rho, alpha)] * (T + 1)] * 4, 2, T, phi=phi, psi=ps)
        if observe:
            _host_observe(hm, 4, last_time=True, softinf=1e2, rng=np.random.default_rng(seed))
        return hm
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


def _hetero_tree(extended=False):
    """extended: with rectangular non-symmetric psi (psi_ji = psi_ij') and two soft observations"""
    T = 2
    A = np.array([[0, 1, 1, 0], [1, 0, 0, 1], [1, 0, 0, 0], [0, 1, 0, 0]])
    qs = [2, 3, 2, 3]
    rng = np.random.default_rng(0)
    phi = [[rng.random(q) + 0.1 for _ in range(T + 1)] for q in qs]
    w = [[M.SISFactor(0.3, 0.2)] * (T + 1) if q == 2 else [M.SIRSFactor(0.3, 0.2, 0.1)] * (T + 1) for q in qs]
    g = M.IndexedBiDiGraph(A)
    ps = None
    if extended:
        base, ps = {}, []
        for (i, j, _) in g.edges():
            key = (min(i, j), max(i, j))
            if key not in base:
                base[key] = [rng.random((qs[key[0]], qs[key[1]])) + 0.2 for _ in range(T + 1)]
            ps.append([m if i < j else m.T.copy() for m in base[key]])
        assert {m[0].shape for m in ps} == {(2, 3), (3, 2), (2, 2), (3, 3)}
        for (i, t, x) in ((1, 2, 2), (2, 1, 0)):     # node i seen in state x at time t, softinf = 30
            phi[i][t] = phi[i][t] * np.where(np.arange(qs[i]) == x, 30.0 / 31.0, 1.0 / 31.0)
    return M.mpbp(g, w, qs, T, phi=phi, psi=ps, max_bond=16)


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


# ================================================================================================ weighted accumulators
# The second half of the sampler - k_weights, k_acc_node, k_acc_pair, k_acc_corr and the four read-outs - against a
# plain high-precision accumulation of the very (X, log w) the device returned.
U = 2.0 ** -53
LDBL = np.longdouble


class _HostModel:
    """What HostSampler reads of an MPBP - graph, factors, states per node, phi and psi in the mirror's padded layout -
    without a device context, so that seeds are chosen and checked where there is no GPU."""

    def __init__(self, g, w, q, T, phi=None, psi=None):
        N = g.nv()
        qn = np.atleast_1d(np.asarray(q, dtype=np.int64))
        self.qnode = (np.full(N, int(qn[0])) if qn.size == 1 else qn).astype(np.int32)
        self.g, self.w, self.q, self.T = g, w, int(self.qnode.max()), int(T)
        self.phi = np.zeros((self.q, T + 1, N))
        self.psi = np.zeros((self.q, self.q, T + 1, g.ne()))
        for i in range(N):
            for t in range(T + 1):
                self.phi[:self.qnode[i], t, i] = 1.0 if phi is None else phi[i][t]
        for (i, j, e) in g.edges():
            for t in range(T + 1):
                self.psi[:self.qnode[i], :self.qnode[j], t, e] = 1.0 if psi is None else psi[e][t]


def _host_observe(hm, nobs, softinf=np.inf, last_time=False, rng=None):
    """draw_node_observations on a _HostModel: the same calls of rng, the prior trajectory from HostSampler"""
    N, T = hm.g.nv(), hm.T
    X, _, near = HostSampler(hm).trajectories(int(rng.integers(0, 2 ** 63 - 1)), [0])
    assert not near.any()
    X = X[0].T + 1
    pairs = [(i, t) for t in (range(T, T + 1) if last_time else range(T + 1)) for i in range(N)]
    observed = sorted(pairs[k] for k in rng.choice(len(pairs), size=int(nobs), replace=False))
    with np.errstate(divide="ignore"):
        lsi = np.log(softinf)
    softone, softzero = 1.0 / (1.0 + np.exp(-lsi)), 1.0 / (1.0 + np.exp(lsi))
    for (i, t) in observed:
        for x in range(hm.qnode[i]):
            hm.phi[x, t, i] *= softone if x == X[i, t] - 1 else softzero
    return X, observed


def _set_inputs(bp, phi=None, psi=None):
    """new phi / psi of a live context: the host mirror, and the device through mpbp_set_phi / mpbp_set_psi"""
    if phi is not None:
        bp.phi[...] = phi
        M._lib.check(bp._L.mpbp_set_phi(bp._h, bp.phi.ravel(order="F").ctypes.data_as(C.POINTER(C.c_double))), bp._h)
    if psi is not None:
        bp.psi[...] = psi
        M._lib.check(bp._L.mpbp_set_psi(bp._h, bp.psi.ravel(order="F").ctypes.data_as(C.POINTER(C.c_double))), bp._h)


class Acc:
    """node[i, t, x], pair[e, t, x_src, x_dst], corr[k, t, u, x_t, x_u] (exactly 0 outside t < u <= t + maxdist; None
    without sites), log sum w, log sum w^2, log ESS.  Probabilities are None where every weight is zero."""

    def __init__(self, node, pair, corr, log_sw, log_sw2, log_ess=None):
        self.node, self.pair, self.corr, self.log_sw, self.log_sw2 = node, pair, corr, log_sw, log_sw2
        self.log_ess = 2 * log_sw - log_sw2 if log_ess is None else log_ess


def _weighted_counts(w, codes, nbins):
    """out[k, ...] = sum_s w[s] [codes[s, ...] == k] in long double, over slabs of samples to bound the temporaries"""
    out = np.zeros((nbins,) + codes.shape[1:], dtype=LDBL)
    step = max(1, (1 << 22) // max(1, int(np.prod(codes.shape[1:]))))
    for a in range(0, len(w), step):
        c, wc = codes[a:a + step], w[a:a + step].reshape((-1,) + (1,) * (codes.ndim - 1))
        for k in range(nbins):
            out[k] += np.add.reduce(np.broadcast_to(wc, c.shape), axis=0, where=(c == k))
    return out


def reference_accumulators(X, logw, ends, q, sites=(), maxdist=None):
    """The importance-weighted marginals of trajectories X [n, T+1, N] (0-based states) with log-weights logw [n]:
    every weight is exp(log w - max log w) in long double (log w = -inf weighs exactly 0), every sum is a long-double
    sum over all n samples at once - no batches, no running maximum, no rescaling.  ends[e] = (src, dst) node of edge e."""
    X = np.asarray(X)
    n, L, N = X.shape
    lw = np.asarray(logw, dtype=LDBL)
    assert lw.shape == (n,) and not np.isnan(lw).any() and not np.isposinf(lw).any()
    top = lw.max()
    ninf = float("-inf")
    if np.isneginf(top):
        return Acc(None, None, None, ninf, ninf, log_ess=ninf)
    with np.errstate(under="ignore"):
        w = np.where(np.isneginf(lw), LDBL(0), np.exp(lw - top))
        w2 = np.where(np.isneginf(lw), LDBL(0), np.exp(2 * (lw - top)))
    sw, sw2 = w.sum(dtype=LDBL), w2.sum(dtype=LDBL)
    log_sw, log_sw2 = top + np.log(sw), 2 * top + np.log(sw2)
    node = np.moveaxis(_weighted_counts(w, X, q), 0, -1) / sw                          # [L, N, q]
    src, dst = np.array([ends[e][0] for e in range(len(ends))]), np.array([ends[e][1] for e in range(len(ends))])
    pc = _weighted_counts(w, X[:, :, src].astype(np.int16) + q * X[:, :, dst], q * q) / sw   # [x_src + q x_dst, L, E]
    pair = pc.reshape(q, q, L, len(ends)).transpose(3, 2, 1, 0)                        # [e, t, x_src, x_dst]
    corr = None
    if len(sites):
        D = L - 1 if maxdist is None else int(maxdist)
        corr = np.zeros((len(sites), L, L, q, q), dtype=LDBL)
        Xs = X[:, :, list(sites)].astype(np.int16)
        for t in range(L):
            for u in range(t + 1, min(L, t + D + 1)):
                cc = _weighted_counts(w, Xs[:, t] + q * Xs[:, u], q * q) / sw         # [x_t + q x_u, k]
                corr[:, t, u] = cc.reshape(q, q, len(sites)).transpose(2, 1, 0)
    f = lambda a: None if a is None else np.asarray(a, dtype=np.float64)
    return Acc(f(node.transpose(1, 0, 2)), f(pair), f(corr), float(log_sw), float(log_sw2),
               log_ess=float(2 * log_sw - log_sw2))


def naive_accumulators(X, logw, ends, q, sites=(), maxdist=None):
    """The same quantities the slowest way: one Python loop over the samples, w = exp(log w) with no shift at all, one
    list of weights per histogram bin, math.fsum of every list."""
    import math
    n, L, N = X.shape
    D = L - 1 if maxdist is None else int(maxdist)
    ws, node, pair, corr = [], {}, {}, {}
    for s in range(n):
        w = math.exp(logw[s])
        ws.append(w)
        for t in range(L):
            for i in range(N):
                node.setdefault((i, t, int(X[s, t, i])), []).append(w)
            for e, (i, j) in enumerate(ends):
                pair.setdefault((e, t, int(X[s, t, i]), int(X[s, t, j])), []).append(w)
            for k, i in enumerate(sites):
                for u in range(t + 1, min(L, t + D + 1)):
                    corr.setdefault((k, t, u, int(X[s, t, i]), int(X[s, u, i])), []).append(w)
    sw, sw2 = math.fsum(ws), math.fsum(w * w for w in ws)
    out = Acc(np.zeros((N, L, q)), np.zeros((len(ends), L, q, q)), np.zeros((len(sites), L, L, q, q)) if len(sites) else None,
              math.log(sw), math.log(sw2))
    for dst, bins in ((out.node, node), (out.pair, pair), (out.corr, corr)):
        for key, lst in bins.items():
            dst[key] = math.fsum(lst) / sw
    return out


def _running_max_steps(logw, calls):
    """increase of the running maximum of log w from the end of one call to the end of the next"""
    ends_ = np.cumsum(calls)
    assert ends_[-1] <= len(logw)
    return np.diff([np.max(logw[:b]) for b in ends_])


def _assert_maximum_moves(logw, calls):
    steps = _running_max_steps(logw, calls)
    assert (steps > 0).sum() >= 2 and steps.max() > np.log(2), steps


SEED_A = 1                  # chosen on the host: test_case_a_seed_moves_the_running_maximum
HARD_OBS_RNG, SEED_HARD = 1, 1   # chosen on the host: test_hard_observation_seed_excludes_sample_zero


def _hard_observed_star(host=False):
    """star of 4, T = 3, psi, two hard observations at the last time (draw_node_observations, softinf = inf)"""
    bp = _star_sis(T=3, psi=True, host=host)
    rng = np.random.default_rng(HARD_OBS_RNG)
    if host:
        _host_observe(bp, 2, last_time=True, rng=rng)
    else:
        M.draw_node_observations(bp, 2, last_time=True, rng=rng)
    return bp


def test_reference_accumulators_match_naive_loop():
    hm = _star_sis(T=3, observe=True, psi=True, host=True)
    X, lw, _ = HostSampler(hm).trajectories(0xACC, np.arange(200))
    assert np.ptp(lw) > 1.0
    lw[[5, 77]] = -np.inf                                    # two excluded trajectories among weighted ones
    ends = [(i, j) for (i, j, _) in hm.g.edges()]
    for sites, md in (([2, 0], 2), ([1], None), ((), None)):
        ref = reference_accumulators(X, lw, ends, 2, sites, md)
        nv = naive_accumulators(X, lw, ends, 2, sites, md)
        for name in ("node", "pair", "corr"):
            a, b = getattr(ref, name), getattr(nv, name)
            assert (a is None and b is None) or np.abs(a - b).max() <= 1e-15, name
        assert abs(ref.node.sum(axis=2) - 1).max() <= 1e-15 and abs(ref.pair.sum(axis=(2, 3)) - 1).max() <= 1e-15
        for name in ("log_sw", "log_sw2", "log_ess"):
            a, b = getattr(ref, name), getattr(nv, name)
            assert abs(a - b) <= 1e-15 * max(1.0, abs(b)), name
    ref = reference_accumulators(X, lw, ends, 2, [2, 0], 2)
    L = hm.T + 1
    for t in range(L):
        for u in range(L):
            if not t < u <= t + 2:
                assert np.all(ref.corr[:, t, u] == 0.0)
            else:                                            # the joint's two margins are the node marginals
                for k, i in enumerate([2, 0]):
                    assert np.abs(ref.corr[k, t, u].sum(axis=1) - ref.node[i, t]).max() <= 1e-15
                    assert np.abs(ref.corr[k, t, u].sum(axis=0) - ref.node[i, u]).max() <= 1e-15
    # far below the range of exp the shift keeps every ratio of weights (log w on a 2^-20 grid: subtracting 5000 is exact)
    lwq = np.round(lw * 2.0 ** 20) / 2.0 ** 20
    ref, deep = (reference_accumulators(X, v, ends, 2, [2, 0], 2) for v in (lwq, lwq - 5000.0))
    assert np.exp(lwq[np.isfinite(lwq)] - 5000.0).max() == 0.0
    assert np.abs(deep.node - ref.node).max() <= 1e-15 and np.abs(deep.corr - ref.corr).max() <= 1e-15
    assert abs(deep.log_sw - (ref.log_sw - 5000.0)) <= 1e-12 and abs(deep.log_ess - ref.log_ess) <= 1e-15
    none = reference_accumulators(X, np.full(200, -np.inf), ends, 2)
    assert none.node is None and none.log_sw == -np.inf and none.log_ess == -np.inf


def test_case_a_seed_moves_the_running_maximum():
    """case A of test_device_accumulators_match_reference: over its calls of 1, 10 and 1000 samples the running maximum of
    log w rises at the end of each of the last two, once by more than log 2 - asserted here from the host restatement."""
    hm = _star_sis(T=3, observe=True, psi=True, host=True)
    _, lw, near = HostSampler(hm).trajectories(SEED_A, np.arange(1011))
    top = [lw[:1].max(), lw[:11].max(), lw.max()]
    assert not near[[int(np.argmax(lw[:b])) for b in (1, 11, 1011)]].any()
    _assert_maximum_moves(lw, (1, 10, 1000))
    assert top[0] < top[1] < top[2]


def test_hard_observation_seed_excludes_sample_zero():
    hm = _hard_observed_star(host=True)
    assert (hm.phi[:, 3, :] == 0).sum() == 2                # two hard observations, at the last time
    _, lw, near = HostSampler(hm).trajectories(SEED_HARD, np.arange(200))
    assert lw[0] == -np.inf and not near[0]
    assert 0.1 < np.isneginf(lw).mean() < 0.9


# ------------------------------------------------------------------------------------------------ GPU: accumulators
def _new_sampler(bp, seed, sites, maxdist):
    return M.SoftMarginSampler(bp, seed=seed, autocorr_sites=sites, maxdist=maxdist)


def _read_device(sms):
    """the four C read-outs of a sampler as an Acc, and the sample count"""
    bp, Lb = sms.bp, sms._L
    N, E, L, q, nc = bp.g.nv(), bp.g.ne(), bp.T + 1, bp.q, len(sms.sites)
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    node, pair, corr = np.full(q * L * N, np.nan), np.full(q * q * L * E, np.nan), np.full(nc * L * L * q * q, np.nan)
    sms._check(Lb.mpbp_sampler_marginals(sms._h, dp(node)))
    sms._check(Lb.mpbp_sampler_pair_marginals(sms._h, dp(pair)))
    if nc:
        sms._check(Lb.mpbp_sampler_twovar_marginals(sms._h, dp(corr)))
    n, a, b = C.c_int64(), C.c_double(), C.c_double()
    sms._check(Lb.mpbp_sampler_counts(sms._h, C.byref(n), C.byref(a), C.byref(b)))
    return Acc(node.reshape(N, L, q), pair.reshape(E, L, q, q).transpose(0, 1, 3, 2),
               corr.reshape(nc, L, L, q, q).transpose(0, 1, 2, 4, 3) if nc else None, a.value, b.value), int(n.value)


def _tolerances(n, ref):
    """Derived, not measured.  A probability is a ratio of two recursive fp64 sums of n non-negative terms, each within
    n u relative (u = 2^-53), hence 4 n u with the two sums' own terms rounded; the floor of 1024 covers the
    |log w - M| u rounding of the exponent's argument and the rescales at batch boundaries.  log sum w adds the rounding
    of M + log(sw), 2^-52 |value|; log ESS = 2 log sum w - log sum w^2 takes three of those."""
    tp = 4 * max(n, 1024) * U
    tl = lambda v: tp + 2.0 ** -52 * abs(v)
    return tp, tl(ref.log_sw), tl(ref.log_sw2), 3 * tl(ref.log_sw)


def _assert_matches(dev, n_dev, ref, n, maxdist, label):
    """every read-out of the device within its derived bound of the reference; the figures are printed first"""
    assert n_dev == n
    tp, tsw, tsw2, tess = _tolerances(n, ref)
    fig = {"node": np.abs(dev.node - ref.node).max(), "pair": np.abs(dev.pair - ref.pair).max(),
           "corr": np.abs(dev.corr - ref.corr).max() if ref.corr is not None else 0.0,
           "log_sw": abs(dev.log_sw - ref.log_sw), "log_sw2": abs(dev.log_sw2 - ref.log_sw2),
           "log_ess": abs(dev.log_ess - ref.log_ess)}
    bound = {"node": tp, "pair": tp, "corr": tp, "log_sw": tsw, "log_sw2": tsw2, "log_ess": tess}
    print(f"[{label}] n = {n}: " + ", ".join(f"{k} {fig[k]:.3e} (bound {bound[k]:.3e})" for k in fig))
    for arr in (dev.node, dev.pair, dev.corr):
        assert arr is None or np.all(np.isfinite(arr))
    assert np.isfinite([dev.log_sw, dev.log_sw2]).all()
    for k in fig:
        assert fig[k] <= bound[k], (label, k, fig[k], bound[k])
    if ref.corr is not None:
        L = ref.corr.shape[1]
        t, u = np.indices((L, L))
        outside = ~((t < u) & (u <= t + maxdist))
        assert np.all(dev.corr[:, outside] == 0.0) and np.all(ref.corr[:, outside] == 0.0)
    return fig


def _karate_observed():
    """_karate_glauber with phi^{t>=1} different at every node, time and state"""
    bp = _karate_glauber()
    phi = bp.phi.copy()
    phi[:, 1:, :] = np.random.default_rng(5).random(phi[:, 1:, :].shape) + 0.2
    _set_inputs(bp, phi=phi)
    return bp


#        model, autocorr sites, maxdist, samples per call on ONE sampler, seed
ACC_CASES = {"A": (lambda: _star_sis(T=3, observe=True, psi=True), [2, 0], 2, (1, 10, 1000, 2 * 65536 + 777), None),
             "B": (lambda: _hetero_tree(extended=True), [3, 1], 1, (7, 65536 + 4321), 0xB0B),
             "C": (_sirs_tree, [0, 1, 2], None, (3000,), 0xC0C),
             "D": (_karate_observed, list(range(34)), 3, (500, 65536 + 123), 0xD0D)}
_acc_runs = {}


def _acc_run(case):
    """one sampler per case, drawn once; its (X, log w), the reference over them and the device read-outs are shared by
    the tests below and left unchanged"""
    if case not in _acc_runs:
        make, sites, md, calls, seed = ACC_CASES[case]
        bp = make()
        sms = _new_sampler(bp, SEED_A if seed is None else seed, sites, md)
        Xs, lws = zip(*(_draw_raw(sms, k) for k in calls))
        X, lw = np.concatenate(Xs), np.concatenate(lws)
        D = bp.T if md is None else md
        ends = [bp._ends[e] for e in range(bp.g.ne())]
        ref = reference_accumulators(X, lw, ends, bp.q, sites, D)
        for a in (X, lw, ref.node, ref.pair, ref.corr):
            a.setflags(write=False)
        dev, n_dev = _read_device(sms)
        _acc_runs[case] = dict(bp=bp, sms=sms, X=X, lw=lw, ref=ref, dev=dev, n_dev=n_dev, calls=calls, D=D, sites=sites)
    return _acc_runs[case]


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(ACC_CASES))
def test_device_accumulators_match_reference(case):
    r = _acc_run(case)
    bp, lw, calls = r["bp"], r["lw"], r["calls"]
    N, E, L, nc = bp.g.nv(), bp.g.ne(), bp.T + 1, len(r["sites"])
    # preconditions: the path this case is here for is live
    assert len(lw) == sum(calls) and np.all(np.isfinite(lw)) and np.ptp(lw) > 0
    if case == "A":
        hm = _star_sis(T=3, observe=True, psi=True, host=True)
        assert np.array_equal(bp.phi, hm.phi) and np.array_equal(bp.psi, hm.psi)
        _assert_maximum_moves(lw, calls)
        assert r["sites"] != sorted(r["sites"]) and r["D"] < bp.T
    if case in "AB":
        assert calls[-1] % 32 != 0 and r["D"] < bp.T
    if case == "A":
        assert calls[-1] > 2 * 65536                         # at least two batch boundaries inside one call
    if case == "B":
        assert sorted(set(int(v) for v in bp.qnode)) == [2, 3] and bp.q == 3
        assert not np.array_equal(bp.psi[:, :, 0, 0], bp.psi[:, :, 0, 0].T)
    if case == "C":
        assert bp.q == 3 and r["D"] == bp.T
    if case == "D":
        assert E == 156 and E * L > 256 and nc * L * r["D"] > 256   # several workgroups of k_acc_pair, k_acc_corr
    _assert_matches(r["dev"], r["n_dev"], r["ref"], len(lw), r["D"], case)


@pytest.mark.gpu
def test_underflowing_weights():
    """log w < -745 for every sample: exp(log w) is 0 in fp64, the sum the reference implementation divides by."""
    bp = _star_sis(T=3, psi=True)
    phi = bp.phi.copy()
    phi[:, 1:, :] = np.array([1e-100, 3e-101])[:, None, None]
    _set_inputs(bp, phi=phi)
    sms = _new_sampler(bp, 41, [0, 3], 3)
    X, lw = _draw_raw(sms, 5000)
    assert lw.max() < -745 and np.all(np.isfinite(lw)) and np.ptp(lw) > 1
    with np.errstate(under="ignore"):
        assert np.exp(lw).sum() == 0.0
    ref = reference_accumulators(X, lw, [bp._ends[e] for e in range(bp.g.ne())], 2, [0, 3], 3)
    dev, n = _read_device(sms)
    _assert_matches(dev, n, ref, 5000, 3, "underflow")
    assert M.effective_sample_size(sms) > 1


@pytest.mark.gpu
def test_hard_observations_zero_weights_then_recovery():
    bp = _hard_observed_star()
    hm = _hard_observed_star(host=True)
    assert np.array_equal(bp.phi, hm.phi) and np.array_equal(bp.psi, hm.psi)
    sms = M.SoftMarginSampler(bp, seed=SEED_HARD, keep_samples=True, autocorr_sites=[1, 0], maxdist=2)
    M.sample(sms, 1)
    assert sms.nsamples == 1 and sms.logw[0] == -np.inf
    n, a, b = C.c_int64(), C.c_double(), C.c_double()
    sms._check(sms._L.mpbp_sampler_counts(sms._h, C.byref(n), C.byref(a), C.byref(b)))
    assert n.value == 1 and a.value == -np.inf and b.value == -np.inf
    assert M.effective_sample_size(sms) == 0.0
    for read in (M.marginals, M.pair_marginals, M.sampling.twovar_marginals):
        with pytest.raises(M.MPBPError) as ei:
            read(sms)
        assert ei.value.code == -1
    M.sample(sms, 20000)
    assert sms.nsamples == 20001 and len(sms.X) == 20001
    zero = np.isneginf(sms.logw)
    assert 0.1 <= zero.mean() <= 0.9 and not np.isnan(sms.logw).any()
    X = np.array(sms.X).transpose(0, 2, 1) - 1
    ref = reference_accumulators(X, sms.logw, [bp._ends[e] for e in range(bp.g.ne())], 2, [1, 0], 2)
    dev, n_dev = _read_device(sms)
    _assert_matches(dev, n_dev, ref, 20001, 2, "hard observations")
    assert abs(np.log(M.effective_sample_size(sms)) - ref.log_ess) <= _tolerances(20001, ref)[3] + 4 * U * abs(ref.log_ess)


@pytest.mark.gpu
def test_inputs_changed_under_a_live_sampler():
    bp = _star_sis(T=3, observe=True, psi=True)
    seed = 0x5EED
    sms = _new_sampler(bp, seed, [0, 1], 2)
    X0, lw0 = _draw_raw(sms, 300)
    rng = np.random.default_rng(9)
    phi, psi = bp.phi.copy(), bp.psi.copy()
    phi[:, 1:, :] = rng.random(phi[:, 1:, :].shape) + 0.1
    for e in range(bp.g.ne()):
        r = int(bp.g.rev[e])
        if e < r:
            psi[:, :, :, e] = rng.random(psi[:, :, :, e].shape) + 0.3
            psi[:, :, :, r] = psi[:, :, :, e].transpose(1, 0, 2)
    assert not np.array_equal(phi, bp.phi) and not np.array_equal(psi, bp.psi)
    _set_inputs(bp, phi=phi, psi=psi)
    X1, lw1 = _draw_raw(sms, 300)
    hX, hlw, near = HostSampler(bp).trajectories(seed, np.arange(300, 600))
    assert near.sum() < 3
    ok = ~near
    assert np.array_equal(X1[ok], hX[ok])
    np.testing.assert_allclose(lw1[ok], hlw[ok], rtol=0, atol=1e-12)
    X, lw = np.concatenate([X0, X1]), np.concatenate([lw0, lw1])
    ref = reference_accumulators(X, lw, [bp._ends[e] for e in range(bp.g.ne())], 2, [0, 1], 2)
    dev, n = _read_device(sms)
    _assert_matches(dev, n, ref, 600, 2, "inputs changed")


# ------------------------------------------------------------------------------------------------ GPU: the Python layer
def _close(a, b, scale):
    """two fp64 evaluations of one formula of at most q^2 = 9 terms of magnitude <= scale: each term and each partial sum
    rounds once in either order, 2 (9 + 9) u scale < 64 u scale; the same relative slack through the square roots"""
    np.testing.assert_allclose(a, b, rtol=64 * U, atol=64 * U * scale)


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["A", "B"])
@pytest.mark.parametrize("fname", ["indicator", "site_dependent"])
def test_python_layer_matches_restatement(case, fname):
    """marginals, pair_marginals, means, autocorrelations, autocovariances and effective_sample_size of sampling.py
    against the reference's definitions (src/sampling.jl:91-185, src/mpbp.jl:288) restated on the raw C read-outs."""
    r = _acc_run(case)
    bp, sms, dev, ref, n = r["bp"], r["sms"], r["dev"], r["ref"], len(r["lw"])
    f = {"indicator": lambda x, i: x - 1, "site_dependent": lambda x, i: (x - 1.75) * (i + 1) + 0.5 * (x == 1)}[fname]
    N, E, L, sites, D = bp.g.nv(), bp.g.ne(), bp.T + 1, r["sites"], r["D"]
    qn = [int(v) for v in bp.qnode]
    sd = lambda p: np.sqrt(np.maximum(p * (1 - p), 0.0) / n)      # n: the count drawn, not the ESS
    assert sms.nsamples == n
    # marginals, pair marginals: the device's numbers, cut to the node's states
    m, me = M.marginals(sms)
    for i in range(N):
        for t in range(L):
            assert np.array_equal(m[i][t], dev.node[i, t, :qn[i]])
            _close(me[i][t], sd(dev.node[i, t, :qn[i]]), 1.0)
    pm, pe = M.pair_marginals(sms)
    for e in range(E):
        i, j = bp._ends[e]
        for t in range(L):
            assert np.array_equal(pm[e][t], dev.pair[e, t, :qn[i], :qn[j]])
            _close(pe[e][t], sd(dev.pair[e, t, :qn[i], :qn[j]]), 1.0)
    # means
    fx = [np.array([f(x + 1, i) for x in range(qn[i])], dtype=float) for i in range(N)]
    F = max(np.abs(v).max() for v in fx)
    mu = [np.array([np.sum(fx[i] * dev.node[i, t, :qn[i]]) for t in range(L)]) for i in range(N)]
    s = [np.array([np.sqrt(np.sum((fx[i] * sd(dev.node[i, t, :qn[i]])) ** 2)) for t in range(L)]) for i in range(N)]
    mv, merr = M.means(f, sms)
    for i in range(N):
        _close(mv[i], mu[i], F)
        _close(merr[i], s[i], F)
    sub = [sites[-1], 0] if 0 not in sites else [0]
    mv2, merr2 = M.means(f, sms, sites=sub)
    for a, i in enumerate(sub):
        _close(mv2[a], mu[i], F)
        _close(merr2[a], s[i], F)
    # autocorrelations and autocovariances: the sampler's own window, then a smaller one (where there is one), the
    # sites reordered, and a subset
    for want_sites, md in ((None, None), (sorted(sites), None), (sites[:1], None), (sorted(sites), 1)):
        d = D if md is None else md
        ss = sites if want_sites is None else want_sites
        rr, re = M.autocorrelations(f, sms, sites=want_sites, maxdist=md)
        cv, ce = M.autocovariances(f, sms, sites=want_sites, maxdist=md)
        assert len(rr) == len(re) == len(cv) == len(ce) == len(ss)
        for a, i in enumerate(ss):
            k = sites.index(i)
            ff = np.outer(fx[i], fx[i])
            r0, e0 = np.zeros((L, L)), np.zeros((L, L))
            for t in range(L):
                for u in range(t + 1, min(L, t + d + 1)):
                    p = dev.corr[k, t, u, :qn[i], :qn[i]]
                    r0[t, u] = np.sum(ff * p)
                    e0[t, u] = np.sqrt(np.sum((ff * sd(p)) ** 2))
            t, u = np.indices((L, L))
            outside = ~((t < u) & (u <= t + d))
            assert np.all(rr[a][outside] == 0.0) and np.all(re[a][outside] == 0.0)
            _close(rr[a], r0, F * F)
            _close(re[a], e0, F * F)
            # covariance(r, mu) = r - mu mu' over the whole matrix; first-order errors
            c0 = r0 - np.outer(mu[i], mu[i])
            ce0 = np.sqrt(e0 ** 2 + np.outer(s[i], mu[i]) ** 2 + np.outer(mu[i], s[i]) ** 2)
            ce0[np.diag_indices(L)] = 2 * np.abs(mu[i]) * s[i]
            _close(cv[a], c0, F * F)
            _close(ce[a], ce0, F * F)
    # the two-time joints the Python layer hands out: None outside the window
    tv = M.sampling.twovar_marginals(sms)
    for k in range(len(sites)):
        for t in range(L):
            for u in range(L):
                if t < u <= t + D:
                    assert np.array_equal(tv[k][t][u], dev.corr[k, t, u])
                else:
                    assert tv[k][t][u] is None
    # effective sample size against the reference's log ESS
    tess = _tolerances(n, ref)[3]
    assert abs(np.log(M.effective_sample_size(sms)) - ref.log_ess) <= tess + 4 * U * abs(ref.log_ess)
