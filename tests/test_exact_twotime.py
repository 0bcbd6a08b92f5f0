"""Exact two-time and alternate marginals on both exact methods (mpbp_exact_twovar_marginals,
mpbp_exact_alternate_marginals; Python `ExactSolver.twovar_marginals`, `.alternate_twovar_marginals`, `exact_beliefs_tu`).

Yardsticks are the enumeration solver's trajectory marginals (`site_marginals`, `alternate_marginals`), oracle/exact.py and
a numpy restatement of the conditioned-vector recursion written here: dense K from the factor callables, masked forward
vectors, b_t.  Tolerances: 1e-9 relative (max abs difference over max abs value) between two fp64 evaluations of the same
sums, 1e-10 on log Z, 1e-8 for MPBP against the exact solver."""
import os
import re

import numpy as np
import pytest

import mpbp_amd as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-9
PATH3 = np.array([[0, 1, 0], [1, 0, 1], [0, 1, 0]])


def _rel(a, b):
    a, b = np.asarray(a, float), np.asarray(b, float)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


def _close(what, a, b, tol=TOL):
    r = _rel(a, b)
    print(f"{what}: max relative difference {r:.3e} (bound {tol:g})")
    assert r < tol, f"{what}: observed max relative difference {r:.3e} (bound {tol:g})"


def _flat_tt(tt):
    """the tables of a `twovar_marginals` / `beliefs_tu` result in order, None entries skipped"""
    return np.concatenate([np.asarray(p, float).ravel() for k in tt for row in k for p in row if p is not None])


def _flat_alt(am):
    return np.concatenate([np.asarray(p, float).ravel() for e in am for p in e])


def _none_pattern(tt):
    return [[[p is None for p in row] for row in k] for k in tt]


# ------------------------------------------------------------------------------------------------ models
def _sym_psi(g, T, qs, pick, rng):
    """psi = 1 except a random positive table on the undirected edge `pick`, at every time (psi_ji = psi_ij')"""
    base = [rng.random((qs[pick[0]], qs[pick[1]])) + 0.3 for _ in range(T + 1)]
    psi = []
    for (i, j, _) in g.edges():
        if (i, j) == pick:
            psi.append([m.copy() for m in base])
        elif (j, i) == pick:
            psi.append([m.T.copy() for m in base])
        else:
            psi.append([np.ones((qs[i], qs[j])) for _ in range(T + 1)])
    return psi


def _ring_adj(N, chord=None):
    A = np.zeros((N, N), dtype=int)
    for i in range(N):
        A[i, (i + 1) % N] = A[(i + 1) % N, i] = 1
    if chord:
        A[chord[0], chord[1]] = A[chord[1], chord[0]] = 1
    return A


def _ring(qs, T, seed, chord=None):
    """SIS (q = 2) / SIRS (q = 3) nodes on a ring (plus a chord) with random positive phi at every time"""
    rng = np.random.default_rng(seed)
    phi = [[rng.random(q) + 0.1 for _ in range(T + 1)] for q in qs]
    w = [[M.SISFactor(0.3, 0.2, 0.02)] * (T + 1) if q == 2 else [M.SIRSFactor(0.3, 0.2, 0.1, 0.05)] * (T + 1) for q in qs]
    return _ring_adj(len(qs), chord), w, phi


def _path3(F):
    """Glauber on the 3-node path, T = 2: a field per node, a table psi on edge (0, 1), a biased phi at t = 0 and a random one
    at t = 1; F is the factor module (device mirror or oracle)"""
    T, h = 2, [0.3, -0.5, 0.8]
    rng = np.random.default_rng(7)
    phi = [[np.array([0.7, 0.3]) if t == 0 else np.ones(2) for t in range(T + 1)] for _ in range(3)]
    phi[2][1] = rng.random(2) + 0.2
    w = [[F.HomogeneousGlauberFactor(1.0, h[i], 0.9)] * (T + 1) for i in range(3)]
    return T, w, phi, rng


def _path3_models():
    from oracle import factors as OF
    from oracle import mpbp as O
    T, w, phi, rng = _path3(M)
    g = M.IndexedBiDiGraph(PATH3)
    psi = _sym_psi(g, T, [2, 2, 2], (0, 1), rng)
    bp = M.mpbp(g, w, 2, T, phi=phi, psi=psi, max_bond=16)
    og = O.IndexedBiDiGraph(PATH3)
    assert [tuple(int(v) for v in e) for e in og.edges()] == bp.g.edges()
    obp = O.mpbp(og, _path3(OF)[1], [2, 2, 2], T, phi=[[bp.phi[:2, t, i].copy() for t in range(T + 1)] for i in range(3)],
                 psi=[[bp.psi[:2, :2, t, e].copy() for t in range(T + 1)] for (i, j, e) in bp.g.edges()])
    return bp, obp


def _mixed_ring():
    T, qs = 2, [2, 3, 2, 3]
    A, w, phi = _ring(qs, T, seed=21)
    g = M.IndexedBiDiGraph(A)
    psi = _sym_psi(g, T, qs, (1, 2), np.random.default_rng(22))
    return M.mpbp(g, w, qs, T, phi=phi, psi=psi, max_bond=4)


def _loopy_long():
    """the 5-node ring plus chord at T = 20 (S = 32) with a hard observation [1, 0] at node 3, time 13, and soft ones"""
    N, T = 5, 20
    A = _ring_adj(N, chord=(0, 2))
    phi = [[np.array([0.8, 0.2]) if t == 0 else np.ones(2) for t in range(T + 1)] for _ in range(N)]
    for (i, t, v) in ((1, 7, [0.1, 0.9]), (3, 13, [1.0, 0.0]), (4, 20, [0.3, 0.7])):
        phi[i][t] = np.array(v)
    w = [[M.SISFactor(0.25, 0.15, 0.02)] * (T + 1) for _ in range(N)]
    return M.mpbp(M.IndexedBiDiGraph(A), w, 2, T, phi=phi, max_bond=4)


# ------------------------------------------------------------------------------------------------ yardsticks
def _tt_of_sites(en, maxdist=None):
    """two-time tables [k][t][u] as axis sums of the enumeration solver's trajectory marginals"""
    L = en.bp.T + 1
    md = L if maxdist is None else maxdist
    return [[[m.sum(axis=tuple(a for a in range(L) if a not in (t, u))) if t < u <= t + md else None for u in range(L)]
             for t in range(L)] for m in en.site_marginals()]


def _numpy_twotime(bp):
    """Two-time tables {(i, t, u): [x_t, x_u]} at every distance and alternate tables {(i, j, t): [x_i^t, x_j^{t+1}]} by the
    recursion over the global state, K built densely from the factor callables w(x', x_nbrs, x)"""
    g, T, N = bp.g, bp.T, bp.g.nv()
    qs = [int(v) for v in bp.qnode]
    st = np.array(list(np.ndindex(*qs)))                 # last node fastest
    S = len(st)
    nbrs = [[int(k) for k in g.neighbors(i)] for i in range(N)]

    def K_of(t):
        K = np.ones((S, S))
        for i in range(N):
            Wi = np.array([[bp.w[i][t](xn + 1, [int(s[k]) + 1 for k in nbrs[i]], int(s[i]) + 1) for xn in range(qs[i])] for s in st])
            K *= Wi[:, st[:, i]]
        return K

    def g_of(t):
        v = np.ones(S)
        for i in range(N):
            v = v * bp.phi[st[:, i], t, i]
        for (i, j, e) in g.edges():
            if i < j:
                v = v * bp.psi[st[:, i], st[:, j], t, e]
        return v

    const = all(all(wt is wi[0] or wt.key() == wi[0].key() for wt in wi) for wi in bp.w)
    Ks = [K_of(0)] * T if const else [K_of(t) for t in range(T)]
    gs = [g_of(t) for t in range(T + 1)]
    a = [None] * (T + 1)
    v = gs[0]
    for t in range(T + 1):
        if t > 0:
            v = gs[t] * (a[t - 1] @ Ks[t - 1])
        a[t] = v / v.sum()
    b = [None] * (T + 1)
    b[T] = np.ones(S)
    for t in range(T - 1, -1, -1):
        v = Ks[t] @ (gs[t + 1] * b[t + 1])
        b[t] = v / v.sum()
    masks = [np.array([(st[:, i] == y).astype(float) for y in range(qs[i])]) for i in range(N)]      # [i][y, s]
    tt, alt = {}, {}
    for t in range(T):
        for i in range(N):
            V = a[t][None, :] * masks[i]
            for u in range(t + 1, T + 1):
                V = gs[u][None, :] * (V @ Ks[u - 1])
                V = V / V.sum()
                tab = (V * b[u][None, :]) @ masks[i].T
                tt[(i, t, u)] = tab / tab.sum()
                if u == t + 1:
                    for j in nbrs[i]:
                        tab = (V * b[u][None, :]) @ masks[j].T
                        alt[(i, j, t)] = tab / tab.sum()
    return tt, alt


def _tt_lists(bp, tt, maxdist=None, nodes=None, shift=0):
    L = bp.T + 1
    md = L if maxdist is None else maxdist
    nodes = range(bp.g.nv()) if nodes is None else nodes
    return [[[tt[(i - shift, t, u)] if t < u <= t + md else None for u in range(L)] for t in range(L)] for i in nodes]


_NUMPY = {}


def _numpy_long():
    """(bp, tt, alt) of the long loopy chain: computed once, shared, never modified"""
    if "long" not in _NUMPY:
        bp = _loopy_long()
        _NUMPY["long"] = (bp,) + _numpy_twotime(bp)
    return _NUMPY["long"]


# ------------------------------------------------------------------------------------------------ 1. CPU
def test_new_names_are_exported_and_declared():
    import importlib
    ex = importlib.import_module("mpbp_amd.exact")
    assert M.exact_beliefs_tu is ex.exact_beliefs_tu
    for name in ("twovar_marginals", "alternate_twovar_marginals"):
        assert callable(getattr(M.ExactSolver, name)), name
    header = open(os.path.join(ROOT, "include", "mpbp_hip.h")).read()
    for name in ("mpbp_exact_twovar_marginals", "mpbp_exact_alternate_marginals"):
        assert name in M._lib.EXPORTS, name
        assert re.search(r"\bint\s+" + name + r"\s*\(\s*mpbp_exact\s*\*", header), name
    import inspect
    for fn in (M.exact_autocorrelations, M.exact_autocovariances):
        assert "maxdist" in inspect.signature(fn).parameters


# ------------------------------------------------------------------------------------------------ 2, 3. against enumeration
def _check_against_enumeration(bp, ac_ref):
    en = M.ExactSolver(bp, "enumerate")
    ref_tt = _tt_of_sites(en)
    ref_alt = en.alternate_marginals()
    f = lambda x, i: M.factors.potts2spin(x) if bp.qnode[i] == 2 else float(x)
    ref_ac = ac_ref(f, en)
    for method in ("transfer", "enumerate"):
        s = M.ExactSolver(bp, method)
        tt = s.twovar_marginals()
        assert _none_pattern(tt) == _none_pattern(ref_tt)
        for k, i in enumerate(range(bp.g.nv())):
            assert all(p.shape == (bp.qnode[i], bp.qnode[i]) for row in tt[k] for p in row if p is not None)
        assert not np.isnan(_flat_tt(tt)).any()
        _close(f"{method}: two-time tables against site_marginals", _flat_tt(tt), _flat_tt(ref_tt))
        am = s.alternate_twovar_marginals()
        assert [[p.shape for p in e] for e in am] == [[p.shape for p in e] for e in ref_alt]
        _close(f"{method}: alternate tables against alternate_marginals", _flat_alt(am), _flat_alt(ref_alt))
        _close(f"{method}: autocorrelations against oracle/exact.py", np.concatenate([r.ravel() for r in s.twovar_autocorrelations(f)]),
               np.concatenate([np.asarray(r).ravel() for r in ref_ac]))
        tt1 = s.twovar_marginals(maxdist=1)
        assert _none_pattern(tt1) == _none_pattern(_tt_of_sites(en, 1))
        _close(f"{method}: maxdist = 1", _flat_tt(tt1), _flat_tt(_tt_of_sites(en, 1)))
    return en


@pytest.mark.gpu
def test_path_of_three_binary_nodes_S8():
    """S = 8 < one MFMA tile, at most 12 rows < 16; the oracle's own enumeration is the source of the autocorrelations"""
    from oracle.exact import exact_autocorrelations, exact_prob
    bp, obp = _path3_models()
    with np.errstate(divide="ignore"):
        po = exact_prob(obp)[0]
    _check_against_enumeration(bp, lambda f, en: exact_autocorrelations(f, obp, po))


@pytest.mark.gpu
def test_mixed_q_ring_S36_and_padding_is_zero():
    """q = [2, 3, 2, 3]: strides that are no powers of two.  oracle/exact.py's autocorrelations are taken of the enumeration
    solver's p (its own enumeration of 46656 trajectories takes minutes)"""
    from oracle.exact import exact_autocorrelations
    bp = _mixed_ring()
    assert int(np.prod(bp.qnode)) == 36
    _check_against_enumeration(bp, lambda f, en: exact_autocorrelations(f, bp, en.prob()))
    L, q, N, E, T = bp.T + 1, bp.q, bp.g.nv(), bp.g.ne(), bp.T
    dp, ip = M._lib.C.POINTER(M._lib.C.c_double), M._lib.C.POINTER(M._lib.C.c_int32)
    for method in ("transfer", "enumerate"):
        s = M.ExactSolver(bp, method)
        nodes = np.arange(N, dtype=np.int32)
        buf = np.full(N * L * L * q * q, np.nan)
        M._lib.check(bp._L.mpbp_exact_twovar_marginals(s._h, nodes.ctypes.data_as(ip), N, 0, buf.ctypes.data_as(dp)), bp._h)
        arr = buf.reshape((N, L, L, q, q))                       # [k][t][u][y][x]
        for i in range(N):
            qi = bp.qnode[i]
            for t in range(L):
                for u in range(L):
                    if t < u:
                        assert (arr[i, t, u, qi:, :] == 0.0).all() and (arr[i, t, u, :, qi:] == 0.0).all()
                        # SIRS forbids some transitions: real entries may be zero, but each table is a distribution
                        assert (arr[i, t, u, :qi, :qi] >= 0.0).all() and abs(arr[i, t, u].sum() - 1.0) < 1e-12
                    else:
                        assert (arr[i, t, u] == 0.0).all()
        buf = np.full(q * q * T * E, np.nan)
        M._lib.check(bp._L.mpbp_exact_alternate_marginals(s._h, buf.ctypes.data_as(dp)), bp._h)
        am = buf.reshape((q, q, T, E), order="F")
        for (i, j, e) in bp.g.edges():
            assert (am[bp.qnode[i]:, :, :, e] == 0.0).all() and (am[:, bp.qnode[j]:, :, e] == 0.0).all()
            assert (am[:bp.qnode[i], :bp.qnode[j], :, e] >= 0.0).all() and np.abs(am[:, :, :, e].sum(axis=(0, 1)) - 1.0).max() < 1e-12


# ------------------------------------------------------------------------------------------------ 4. time-dependent factors
@pytest.mark.gpu
def test_time_dependent_factors_against_enumeration():
    """4 binary nodes on a ring, T = 4, SIS rates that differ per time: Q = 2^20 trajectories are still enumerated, and the
    Kronecker halves of K_t are rebuilt at every step of the conditioned vectors"""
    N, T = 4, 4
    rng = np.random.default_rng(41)
    phi = [[rng.random(2) + 0.1 for _ in range(T + 1)] for _ in range(N)]
    w = [[M.SISFactor(0.2 + 0.07 * t, 0.1 + 0.05 * t, 0.02) for t in range(T + 1)] for _ in range(N)]
    bp = M.mpbp(M.IndexedBiDiGraph(_ring_adj(N)), w, 2, T, phi=phi, max_bond=4)
    assert bp.w[0][0].key() != bp.w[0][1].key()
    en, tr = M.ExactSolver(bp, "enumerate"), M.ExactSolver(bp, "transfer")
    d = abs(tr.logZ - en.logZ)
    assert d < 1e-10, f"logZ: observed difference {d:.3e}"
    _close("two-time tables", _flat_tt(tr.twovar_marginals()), _flat_tt(_tt_of_sites(en)))
    _close("two-time tables, maxdist = 2", _flat_tt(tr.twovar_marginals(maxdist=2)), _flat_tt(_tt_of_sites(en, 2)))
    _close("alternate tables", _flat_alt(tr.alternate_twovar_marginals()), _flat_alt(en.alternate_marginals()))


# ------------------------------------------------------------------------------------------------ 5. long chain
@pytest.mark.gpu
@pytest.mark.parametrize("maxdist", [1, 5, None])
def test_long_loopy_chain_matches_numpy_recursion(maxdist):
    bp, ntt, nalt = _numpy_long()
    assert int(np.prod(bp.qnode)) == 32 and bp.T == 20
    s = M.ExactSolver(bp, "transfer")
    tt = s.twovar_marginals(maxdist=maxdist)
    ref = _tt_lists(bp, ntt, maxdist)
    assert _none_pattern(tt) == _none_pattern(ref)
    assert not np.isnan(_flat_tt(tt)).any()
    _close("two-time tables", _flat_tt(tt), _flat_tt(ref))
    # node 3 is observed in state 0 at t = 13: the excluded state's row (origin) and column (read-out) are exactly zero
    md = bp.T if maxdist is None else maxdist
    for u in range(14, min(bp.T, 13 + md) + 1):
        assert (tt[3][13][u][1, :] == 0.0).all() and (tt[3][13][u][0, :] > 0.0).all()
    for t in range(max(0, 13 - md), 13):
        assert (tt[3][t][13][:, 1] == 0.0).all() and (tt[3][t][13][:, 0] > 0.0).all()
    am = s.alternate_twovar_marginals()
    assert not np.isnan(_flat_alt(am)).any()
    _close("alternate tables", _flat_alt(am), _flat_alt([[nalt[(i, j, t)] for t in range(bp.T)] for (i, j, e) in bp.g.edges()]))
    for (i, j, e) in bp.g.edges():
        if i == 3:
            assert (am[e][13][1, :] == 0.0).all()
        if j == 3:
            assert (am[e][12][:, 1] == 0.0).all()


# ------------------------------------------------------------------------------------------------ 6. many tiles and chunks
@pytest.mark.gpu
def test_many_tiles_factorise_over_components():
    """S = 72 x 144 = 10368: ragged 64-column tiles of the batched step, 162 column tiles, 648 k-steps; the tables of the union of
    two disconnected components are those of the components, which the numpy recursion gives at S = 72 and S = 144"""
    T = 3
    parts = [_ring([2, 3, 2, 3, 2], T, seed=31, chord=(0, 2)), _ring([3, 2, 2, 3, 2, 2], T, seed=32)]
    ref_tt, ref_alt, n0 = [], {}, parts[0][0].shape[0]
    for c, (A, w, phi) in enumerate(parts):
        qs = [len(p[0]) for p in phi]
        cbp = M.mpbp(M.IndexedBiDiGraph(A), w, qs, T, phi=phi, max_bond=4)
        tt, alt = _numpy_twotime(cbp)
        ref_tt += _tt_lists(cbp, tt)
        ref_alt.update({(i + c * n0, j + c * n0, t): v for (i, j, t), v in alt.items()})
    A = np.zeros((11, 11), dtype=int)
    A[:n0, :n0], A[n0:, n0:] = parts[0][0], parts[1][0]
    w, phi = parts[0][1] + parts[1][1], parts[0][2] + parts[1][2]
    qs = [len(p[0]) for p in phi]
    assert int(np.prod(qs)) == 10368
    bp = M.mpbp(M.IndexedBiDiGraph(A), w, qs, T, phi=phi, max_bond=4)
    s = M.ExactSolver(bp, "transfer")
    tt = s.twovar_marginals()
    assert _none_pattern(tt) == _none_pattern(ref_tt)
    _close("two-time tables", _flat_tt(tt), _flat_tt(ref_tt))
    _close("alternate tables", _flat_alt(s.alternate_twovar_marginals()),
           _flat_alt([[ref_alt[(i, j, t)] for t in range(T)] for (i, j, e) in bp.g.edges()]))


# ------------------------------------------------------------------------------------------------ 7. batching, bit for bit
@pytest.mark.gpu
def test_results_do_not_depend_on_the_batching(monkeypatch):
    bp = _loopy_long()
    monkeypatch.delenv("MPBP_EXACT_TT_ROWS", raising=False)
    s = M.ExactSolver(bp, "transfer")
    full, full2 = s.twovar_marginals(), s.twovar_marginals(maxdist=2)
    alt = s.alternate_twovar_marginals()
    one = s.twovar_marginals(sites=[2], maxdist=2)
    assert len(one) == 1 and _none_pattern(one) == _none_pattern([full2[2]])
    assert np.array_equal(_flat_tt(one), _flat_tt([full2[2]]))
    cut = [[[p if (p is not None and u <= t + 2) else None for u, p in enumerate(row)] for t, row in enumerate(full[2])]]
    assert np.array_equal(_flat_tt(one), _flat_tt(cut))
    monkeypatch.setenv("MPBP_EXACT_TT_ROWS", "5")            # two nodes per pass, one origin time per pass
    assert np.array_equal(_flat_tt(s.twovar_marginals()), _flat_tt(full))
    assert np.array_equal(_flat_tt(s.twovar_marginals(maxdist=2)), _flat_tt(full2))
    assert np.array_equal(_flat_alt(s.alternate_twovar_marginals()), _flat_alt(alt))
    monkeypatch.setenv("MPBP_EXACT_TT_ROWS", "37")           # a ragged last row tile, three origin times per pass
    assert np.array_equal(_flat_tt(s.twovar_marginals()), _flat_tt(full))
    monkeypatch.delenv("MPBP_EXACT_TT_ROWS")
    s2 = M.ExactSolver(bp, "transfer")
    assert np.array_equal(_flat_tt(s2.twovar_marginals()), _flat_tt(full))
    assert np.array_equal(_flat_alt(s2.alternate_twovar_marginals()), _flat_alt(alt))
    assert s2.logZ == s.logZ


# ------------------------------------------------------------------------------------------------ 8. MPBP against the truth
@pytest.mark.gpu
def test_mpbp_two_time_observables_on_a_tree_are_exact_at_T10():
    """SIS on the 5-node tree at T = 10 with nothing truncated away: the engine's beliefs_tu, autocorrelations and alternate
    marginals are those of the exact solver.  Q = 2^55: the enumeration is refused, the module functions transfer"""
    T, N, max_bond = 10, 5, 64
    A = np.zeros((N, N), dtype=int)
    for (i, j) in ((0, 1), (1, 2), (1, 3), (3, 4)):
        A[i, j] = A[j, i] = 1
    phi = [[np.array([0.7, 0.3]) if t == 0 else np.ones(2) for t in range(T + 1)] for _ in range(N)]
    phi[2][6] = np.array([0.2, 0.8])
    phi[4][T] = np.array([0.9, 0.1])
    bp = M.mpbp(M.IndexedBiDiGraph(A), [[M.SISFactor(0.3, 0.2, 0.05)] * (T + 1)] * N, 2, T, phi=phi, max_bond=max_bond)
    M.iterate(bp, maxiter=12, svd_trunc=M.TruncThresh(1e-14), tol=1e-13, schedule="colored")
    st = bp.last_stats
    assert st.nan_flag == 0 and st.capacity_flag == 0
    top = int(bp.bonds().max())
    assert top < max_bond, f"largest bond {top} reached the capacity {max_bond}"
    with pytest.raises(M.MPBPError) as ei:
        M.ExactSolver(bp, "enumerate")
    assert ei.value.code == -4
    f = lambda x, i: M.factors.potts2spin(x)
    tt = M.exact_beliefs_tu(bp)
    btu = M.beliefs_tu(bp)
    assert _none_pattern(tt) == _none_pattern(btu)
    _close("beliefs_tu", _flat_tt(btu), _flat_tt(tt), 1e-8)
    _close("beliefs_tu, sites and maxdist", _flat_tt(M.beliefs_tu(bp, sites=[3, 0], maxdist=4)),
           _flat_tt(M.exact_beliefs_tu(bp, sites=[3, 0], maxdist=4)), 1e-8)
    _close("autocorrelations", np.array(M.autocorrelations(f, bp)), np.array(M.exact_autocorrelations(f, bp)), 1e-8)
    _close("autocorrelations, maxdist = 3", np.array(M.autocorrelations(f, bp, maxdist=3)),
           np.array(M.exact_autocorrelations(f, bp, maxdist=3)), 1e-8)
    _close("autocovariances", np.array(M.autocovariances(f, bp)), np.array(M.exact_autocovariances(f, bp)), 1e-8)
    am, ex = M.alternate_marginals(bp), M.exact_alternate_marginals(bp)
    _close("alternate marginals", _flat_alt([am[e] for e in range(bp.g.ne())]), _flat_alt(ex), 1e-8)
    s = M.ExactSolver(bp, "transfer")
    _close("a transfer solver passed as p_exact", np.array(M.exact_autocorrelations(f, bp, p_exact=s)),
           np.array(M.exact_autocorrelations(f, bp)), 1e-12)


# ------------------------------------------------------------------------------------------------ 9. refusals and refresh
@pytest.mark.gpu
def test_bad_node_is_refused_and_new_observations_are_seen():
    T = 3
    rng = np.random.default_rng(9)
    phi = [[rng.random(2) + 0.1 for _ in range(T + 1)] for _ in range(3)]
    bp = M.mpbp(M.IndexedBiDiGraph(PATH3), [[M.SISFactor(0.3, 0.2, 0.05)] * (T + 1)] * 3, 2, T, phi=phi, max_bond=4)
    for method in ("transfer", "enumerate"):
        s = M.ExactSolver(bp, method)
        for bad in ([3], [0, -1]):
            with pytest.raises(M.MPBPError) as ei:
                s.twovar_marginals(sites=bad)
            assert ei.value.code == -1 and "out of range" in str(ei.value)
        assert np.isfinite(s.logZ)
        _close(f"{method}: after the refusal", _flat_tt(s.twovar_marginals()), _flat_tt(_tt_of_sites(M.ExactSolver(bp, "enumerate"))))
        assert s.twovar_marginals(maxdist=0) == [[[None] * (T + 1)] * (T + 1)] * 3
    s = M.ExactSolver(bp, "transfer")
    before, before_alt = _flat_tt(s.twovar_marginals()), _flat_alt(s.alternate_twovar_marginals())
    M.reset_observations(bp)
    en = M.ExactSolver(bp, "enumerate")
    after = _flat_tt(s.twovar_marginals())
    assert _rel(after, before) > 1e-3
    _close("two-time tables of the new phi", after, _flat_tt(_tt_of_sites(en)))
    after_alt = _flat_alt(s.alternate_twovar_marginals())
    assert _rel(after_alt, before_alt) > 1e-3
    _close("alternate tables of the new phi", after_alt, _flat_alt(en.alternate_marginals()))
