"""Exact solvers on the device (mpbp_exact_*, csrc/exact.hip; reference src/exact.jl): joint enumeration against the golden
enumeration fixture and against oracle/exact.py element by element, the global-state transfer solver against enumeration
and against a forward-backward restated here in numpy from the factor callables, MPBP against the truth at T = 10.

Tolerance: two fp64 evaluations of the same sums of at most 2^16 non-negative terms differ by at most n eps ~ 7e-12
relative; the comparisons use 1e-9 (max abs difference over max abs value, `_rel` of tests/test_gpu_parity.py)."""
import os

import numpy as np
import pytest

import mpbp_amd as M

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TOL = 1e-9
PATH3 = np.array([[0, 1, 0], [1, 0, 1], [0, 1, 0]])
STAR4 = np.array([[0, 1, 1, 1], [1, 0, 0, 0], [1, 0, 0, 0], [1, 0, 0, 0]])


def _flat(bb):
    return np.concatenate([np.asarray(p, float).ravel() for b in bb for p in b])


def _rel(a, b):
    a, b = np.asarray(a, float), np.asarray(b, float)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


def _close(what, a, b, tol=TOL):
    r = _rel(a, b)
    assert r < tol, f"{what}: observed max relative difference {r:.3e} (bound {tol:g})"


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


def _glauber_path(F, variant):
    """cases (a), (c), (d), (f): Glauber on the 3-node path, T = 2, a different field per node, a table psi on edge (0, 1),
    a biased phi at t = 0 and a random phi at t = 1; F is the factor module (device mirror or oracle)."""
    T, h = 2, [0.3, -0.5, 0.8]
    rng = np.random.default_rng(7)
    phi = [[np.array([0.7, 0.3]) if t == 0 else np.ones(2) for t in range(T + 1)] for _ in range(3)]
    phi[2][1] = rng.random(2) + 0.2
    if variant == "f":
        phi[1][1] = np.array([1.0, 0.0])
    betas = [0.6, 1.1, 1.7] if variant == "c" else [0.9] * 3
    ws = {b: [F.HomogeneousGlauberFactor(1.0, h[i], b) for i in range(3)] for b in set(betas)}
    w = [[ws[betas[t]][i] for t in range(T + 1)] for i in range(3)]
    return T, w, phi, rng


def _case(name):
    """(device MPBP, oracle factor lists, periodic) of a test case"""
    from oracle import factors as OF
    if name in "acdf":
        T, w, phi, rng = _glauber_path(M, name)
        ow = _glauber_path(OF, name)[1]
        g = M.IndexedBiDiGraph(PATH3)
        psi = _sym_psi(g, T, [2, 2, 2], (0, 1), rng)
        make = M.periodic_mpbp if name == "d" else M.mpbp
        bp = make(g, w, 2, T, phi=phi, psi=psi, max_bond=16)
        if name == "c":
            assert bp.w[0][0].key() != bp.w[0][1].key()
        return bp, ow, name == "d"
    if name == "b":
        T, qs = 2, [2, 3, 2]
        rng = np.random.default_rng(11)
        phi = [[rng.random(q) + 0.1 for _ in range(T + 1)] for q in qs]
        mk = lambda F: [[F.SISFactor(0.3 + 0.1 * i, 0.2)] * (T + 1) if q == 2 else [F.SIRSFactor(0.35, 0.25, 0.15, 0.05)] * (T + 1)
                        for i, q in enumerate(qs)]
        g = M.IndexedBiDiGraph(PATH3)
        psi = _sym_psi(g, T, qs, (1, 2), rng)
        return M.mpbp(g, mk(M), qs, T, phi=phi, psi=psi, max_bond=16), mk(OF), False
    if name == "e":
        T = 2
        J = STAR4 * np.array([[0, 0.7, -0.4, 1.3]] * 4)
        J = J + J.T
        h = np.array([0.2, -0.3, 0.5, 0.1])
        rng = np.random.default_rng(5)
        phi = [[np.array([0.6, 0.4]) if t == 0 else rng.random(2) + 0.2 for t in range(T + 1)] for _ in range(4)]
        w, ow = M.glauber_factors(J != 0, J, h, 0.8, T), OF.glauber_factors(J != 0, J, h, 0.8, T)
        assert isinstance(w[0][0], M.GenericGlauberFactor)
        return M.mpbp(M.IndexedBiDiGraph(J != 0), w, 2, T, phi=phi, max_bond=4), ow, False
    if name == "star":
        d = np.load(os.path.join(GOLD, "sis_star4_T3_exact.npz"))
        return _golden_model(d), [[OF.SISFactor(*d["params"][1:3], d["params"][4])] * (int(d["params"][0]) + 1)] * 4, False
    raise KeyError(name)


def _golden_model(d):
    T, lam, rho, gam, alpha = d["params"]
    T = int(T)
    phi = [[d["phi"][i, t] for t in range(T + 1)] for i in range(4)]
    return M.mpbp(M.IndexedBiDiGraph(d["A"]), [[M.SISFactor(lam, rho, alpha)] * (T + 1)] * 4, 2, T, phi=phi, max_bond=16)


def _oracle_of(bp, factors):
    """the oracle model of a device MPBP: same graph, the oracle's factors, the device model's phi and psi"""
    from oracle import mpbp as O
    A = np.zeros((bp.g.nv(), bp.g.nv()), dtype=int)
    for (i, j, _) in bp.g.edges():
        A[i, j] = 1
    og = O.IndexedBiDiGraph(A)
    assert [tuple(int(v) for v in e) for e in og.edges()] == bp.g.edges()
    qs = [int(v) for v in bp.qnode]
    phi = [[bp.phi[:qs[i], t, i].copy() for t in range(bp.T + 1)] for i in range(bp.g.nv())]
    psi = [[bp.psi[:qs[i], :qs[j], t, e].copy() for t in range(bp.T + 1)] for (i, j, e) in bp.g.edges()]
    return O.mpbp(og, factors, qs, bp.T, phi=phi, psi=psi)


_ORACLE = {}


def _oracle(name):
    """(obp, p, Z) of oracle/exact.py for a case: computed once, shared, never modified"""
    if name not in _ORACLE:
        from oracle.exact import exact_prob
        bp, ow, periodic = _case(name)
        obp = _oracle_of(bp, ow)
        with np.errstate(divide="ignore"):
            p, Z = exact_prob(obp, periodic=periodic)
        p.setflags(write=False)
        _ORACLE[name] = (obp, p, Z)
    return _ORACLE[name]


# ------------------------------------------------------------------------------------------------ 9. CPU
def test_module_exports_and_auto_rule():
    import importlib
    ex = importlib.import_module("mpbp_amd.exact")
    for name in ["ExactSolver", "exact_prob", "site_marginals", "exact_marginals", "exact_pair_marginals",
                 "exact_alternate_marginals", "exact_autocorrelations", "exact_autocovariances", "exact_marginal_expectations",
                 "exact_pair_marginal_expectations", "exact_alternate_marginal_expectations"]:
        assert getattr(M, name) is getattr(ex, name), name
    for name in ["mpbp_exact_create", "mpbp_exact_destroy", "mpbp_exact_solve", "mpbp_exact_marginals", "mpbp_exact_pair_marginals",
                 "mpbp_exact_prob", "mpbp_exact_set_prob", "mpbp_exact_site_marginals", "mpbp_exact_edge_marginals"]:
        assert name in M._lib.EXPORTS
    assert "exact.hip" in M._lib.SOURCES
    # (N, T, q): Q = 2^24 <= 2^26 enumerates; Q = 2^30 transfers (S = 2^5); Q = 2^34, S = 2^17 has no method
    assert ex.choose_method([2] * 4, 5) == "enumerate"
    assert ex.choose_method([2] * 5, 5) == "transfer"
    assert ex.choose_method([2] * 12, 50) == "transfer"
    with pytest.raises(M.MPBPError) as ei:
        ex.choose_method([2] * 17, 1)
    assert ei.value.code == -4
    with pytest.raises(M.MPBPError):
        ex.choose_method([2] * 5, 5, periodic=True)
    assert M.pair_marginals is M.sampling.pair_marginals if hasattr(M, "sampling") else True


# ------------------------------------------------------------------------------------------------ 1. golden
@pytest.mark.gpu
@pytest.mark.parametrize("method", ["enumerate", "transfer"])
def test_golden_enumeration_fixture(method):
    d = np.load(os.path.join(GOLD, "sis_star4_T3_exact.npz"))
    s = M.ExactSolver(_golden_model(d), method)
    _close("marginals", np.array(M.exact_marginals(s.bp, p_exact=s)), d["marginals"])
    _close("pair marginals", np.array(M.exact_pair_marginals(s.bp, p_exact=s)), d["pair_marginals"])
    _close("Z", s.Z, float(d["Z"]))


# ------------------------------------------------------------------------------------------------ 2. enumeration vs oracle
@pytest.mark.gpu
@pytest.mark.parametrize("name", ["a", "b", "c", "d", "e", "f"])
def test_enumeration_matches_oracle(name):
    from oracle.exact import exact_autocorrelations, exact_marginals, exact_pair_marginals
    obp, po, Zo = _oracle(name)
    bp = _case(name)[0]
    p, Z = M.exact_prob(bp)
    assert p.shape == po.shape
    assert not np.isnan(p).any()
    _close("p, element by element", p, po)
    _close("Z", Z, Zo)
    assert ((po == 0.0) == (p == 0.0)).all()
    if name == "f":
        # node 1 observed in state 0 at t = 1: digit 1 (T+1) + 1 of the configuration
        excl = np.take(p, 1, axis=1 * (bp.T + 1) + 1)
        assert excl.size == p.size // 2 and (excl == 0.0).all()
    s = M.ExactSolver(bp, "enumerate")
    _close("marginals", _flat(s.marginals()), _flat(exact_marginals(obp, po)))
    _close("pair marginals", _flat(s.pair_marginals()), _flat(exact_pair_marginals(obp, po)))
    f = lambda x, i: M.factors.potts2spin(x)
    _close("autocorrelations", np.array(s.autocorrelations(f)), np.array(exact_autocorrelations(f, obp, po)))
    # the same reductions on an uploaded p (mpbp_exact_set_prob), through the reference's names
    _close("marginals of a loaded p", _flat(M.exact_marginals(bp, p_exact=p)), _flat(exact_marginals(obp, po)))
    if name == "b":
        buf = np.full(bp.q * (bp.T + 1) * 3, np.nan)
        M._lib.check(bp._L.mpbp_exact_marginals(s._h, buf.ctypes.data_as(M._lib.C.POINTER(M._lib.C.c_double))), bp._h)
        m = buf.reshape((3, bp.T + 1, 3), order="F")
        assert (m[2, :, 0] == 0.0).all() and (m[2, :, 2] == 0.0).all() and (m[2, :, 1] > 0.0).all()
        buf = np.full(9 * (bp.T + 1) * bp.g.ne(), np.nan)
        M._lib.check(bp._L.mpbp_exact_pair_marginals(s._h, buf.ctypes.data_as(M._lib.C.POINTER(M._lib.C.c_double))), bp._h)
        pm = buf.reshape((3, 3, bp.T + 1, bp.g.ne()), order="F")
        for (i, j, e) in bp.g.edges():
            assert (pm[bp.qnode[i]:, :, :, e] == 0.0).all() and (pm[:, bp.qnode[j]:, :, e] == 0.0).all()
            assert (pm[:bp.qnode[i], :bp.qnode[j], :, e] > 0.0).all()


@pytest.mark.gpu
def test_site_and_edge_trajectory_marginals():
    """mpbp_exact_site_marginals / mpbp_exact_edge_marginals on the mixed-q case against axis sums of the oracle's p; an
    edge i -> j with i > j comes indexed [traj_i, traj_j] all the same"""
    obp, po, _ = _oracle("b")
    bp = _case("b")[0]
    s = M.ExactSolver(bp, "enumerate")
    L = bp.T + 1
    for i, m in enumerate(s.site_marginals()):
        ref = po.sum(axis=tuple(a for a in range(3 * L) if a // L != i))
        assert m.shape == ref.shape
        _close(f"site {i}", m, ref)
    for (i, j, e), m in zip(bp.g.edges(), s.edge_marginals()):
        ref = po.sum(axis=tuple(a for a in range(3 * L) if a // L not in (i, j)))
        if i > j:
            ref = np.moveaxis(ref, list(range(L)), list(range(L, 2 * L)))
        assert m.shape == ref.shape
        _close(f"edge {i}->{j}", m, ref)


# ------------------------------------------------------------------------------------------------ 3. alternate marginals
@pytest.mark.gpu
def test_alternate_marginals_match_axis_sums():
    obp, po, _ = _oracle("a")
    bp = _case("a")[0]
    am = M.exact_alternate_marginals(bp)
    L = bp.T + 1
    for (i, j, e) in bp.g.edges():
        for t in range(L - 1):
            a, b = i * L + t, j * L + t + 1
            ref = po.sum(axis=tuple(c for c in range(po.ndim) if c not in (a, b)))
            _close(f"edge {i}->{j} t = {t}", am[e][t], ref if a < b else ref.T)
    ex = M.exact_alternate_marginal_expectations(lambda x, e: M.factors.potts2spin(x), bp)
    fx = np.array([1.0, -1.0])
    assert abs(ex[0][0] - fx @ am[0][0] @ fx) < 1e-14


# ------------------------------------------------------------------------------------------------ 4. transfer vs enumeration
@pytest.mark.gpu
@pytest.mark.parametrize("name", ["a", "b", "c", "e", "star"])
def test_transfer_matches_enumeration(name):
    bp = _case(name)[0]
    en, tr = M.ExactSolver(bp, "enumerate"), M.ExactSolver(bp, "transfer")
    d = abs(tr.logZ - en.logZ)
    assert d < 1e-10, f"logZ: observed difference {d:.3e}"
    _close("marginals", _flat(tr.marginals()), _flat(en.marginals()))
    _close("pair marginals", _flat(tr.pair_marginals()), _flat(en.pair_marginals()))


def _ring(qs, T, seed, chord=None):
    """SIS (q = 2) / SIRS (q = 3) nodes on a ring (plus a chord) with random positive phi at every time"""
    N = len(qs)
    A = np.zeros((N, N), dtype=int)
    for i in range(N):
        A[i, (i + 1) % N] = A[(i + 1) % N, i] = 1
    if chord:
        A[chord[0], chord[1]] = A[chord[1], chord[0]] = 1
    rng = np.random.default_rng(seed)
    phi = [[rng.random(q) + 0.1 for _ in range(T + 1)] for q in qs]
    w = [[M.SISFactor(0.3, 0.2, 0.02)] * (T + 1) if q == 2 else [M.SIRSFactor(0.3, 0.2, 0.1, 0.05)] * (T + 1) for q in qs]
    return A, w, phi


@pytest.mark.gpu
@pytest.mark.parametrize("qs,T", [([2, 2, 2, 2], 4), ([2, 3, 2, 3], 2)])
def test_enumeration_over_many_chunks_matches_transfer(qs, T):
    """Q = 2^20 and Q = 8 27 8 27 = 46656 configurations: more than one 4096-element chunk in the normalisation and more
    than one piece per bin in the strided reductions (with strides that are powers of two, and that are not).  The sums have
    up to 2^20 terms, each a tree over fixed pieces: the error stays far below 1e-9."""
    A, w, phi = _ring(qs, T, seed=21)
    bp = M.mpbp(M.IndexedBiDiGraph(A), w, qs, T, phi=phi, max_bond=4)
    en, tr = M.ExactSolver(bp, "enumerate"), M.ExactSolver(bp, "transfer")
    d = abs(tr.logZ - en.logZ)
    assert d < 1e-10, f"logZ: observed difference {d:.3e}"
    _close("marginals", _flat(en.marginals()), _flat(tr.marginals()))
    _close("pair marginals", _flat(en.pair_marginals()), _flat(tr.pair_marginals()))
    L = T + 1
    for i, m in enumerate(en.site_marginals()):
        for t in (0, T):
            _close(f"site {i} t = {t}", m.sum(axis=tuple(a for a in range(L) if a != t)), tr.marginals()[i][t])


@pytest.mark.gpu
def test_transfer_over_many_tiles_factorises_over_components():
    """S = 72 x 144 = 10368 global states: KA / KB wider than one 64-column tile with ragged edges, 41 chunks of 256 states
    in the forward product (the last one partial).  The graph is two disconnected components, so log Z is the sum and the
    marginals are those of the components solved on their own (S = 72 and 144: one tile, checked against enumeration above)"""
    T = 3
    parts = [_ring([2, 3, 2, 3, 2], T, seed=31, chord=(0, 2)), _ring([3, 2, 2, 3, 2, 2], T, seed=32)]
    solo = []
    for (A, w, phi) in parts:
        qs = [len(p[0]) for p in phi]
        solo.append(M.ExactSolver(M.mpbp(M.IndexedBiDiGraph(A), w, qs, T, phi=phi, max_bond=4), "transfer"))
    n0 = parts[0][0].shape[0]
    A = np.zeros((11, 11), dtype=int)
    A[:n0, :n0], A[n0:, n0:] = parts[0][0], parts[1][0]
    w, phi = parts[0][1] + parts[1][1], parts[0][2] + parts[1][2]
    qs = [len(p[0]) for p in phi]
    assert int(np.prod(qs)) == 10368
    s = M.ExactSolver(M.mpbp(M.IndexedBiDiGraph(A), w, qs, T, phi=phi, max_bond=4), "transfer")
    d = abs(s.logZ - (solo[0].logZ + solo[1].logZ))
    assert d < 1e-10, f"logZ: observed difference {d:.3e}"
    _close("marginals", _flat(s.marginals()), _flat(solo[0].marginals() + solo[1].marginals()))
    _close("pair marginals", _flat(s.pair_marginals()), _flat(solo[0].pair_marginals() + solo[1].pair_marginals()))


# ------------------------------------------------------------------------------------------------ 5. transfer at long T
def _numpy_forward_backward(bp):
    """log Z, node marginals [i][t] and pair marginals [e][t] by the forward-backward recursion over the global state, with
    the dense K built from the factor callables w(x', x_nbrs, x) - nothing of the dense-table fold is used"""
    g, T, N = bp.g, bp.T, bp.g.nv()
    qs = [int(v) for v in bp.qnode]
    states = list(np.ndindex(*qs))                 # last node fastest
    S = len(states)
    nbrs = [[int(k) for k in g.neighbors(i)] for i in range(N)]

    def K_of(t):
        K = np.ones((S, S))
        for a, s in enumerate(states):
            for i in range(N):
                col = [bp.w[i][t](xn + 1, [s[k] + 1 for k in nbrs[i]], s[i] + 1) for xn in range(qs[i])]
                for b, sn in enumerate(states):
                    K[a, b] *= col[sn[i]]
        return K

    def g_of(t):
        v = np.ones(S)
        for a, s in enumerate(states):
            for i in range(N):
                v[a] *= bp.phi[s[i], t, i]
            for (i, j, e) in g.edges():
                if i < j:
                    v[a] *= bp.psi[s[i], s[j], t, e]
        return v

    const = all(all(wt is wi[0] or wt.key() == wi[0].key() for wt in wi) for wi in bp.w)
    Ks = [K_of(0)] * T if const else [K_of(t) for t in range(T)]
    gs = [g_of(t) for t in range(T + 1)]
    a, logZ = [None] * (T + 1), 0.0
    v = gs[0]
    for t in range(T + 1):
        if t > 0:
            v = gs[t] * (a[t - 1] @ Ks[t - 1])
        z = v.sum()
        a[t], logZ = v / z, logZ + np.log(z)
    b = np.ones(S)
    gam = [None] * (T + 1)
    for t in range(T, -1, -1):
        if t < T:
            b = Ks[t] @ (gs[t + 1] * b)
            b = b / b.sum()
        gam[t] = a[t] * b / (a[t] * b).sum()
    idx = np.array(states)
    marg = [[np.array([gam[t][idx[:, i] == x].sum() for x in range(qs[i])]) for t in range(T + 1)] for i in range(N)]
    pair = [[np.array([[gam[t][(idx[:, i] == x) & (idx[:, j] == y)].sum() for y in range(qs[j])] for x in range(qs[i])])
             for t in range(T + 1)] for (i, j, e) in g.edges()]
    return logZ, marg, pair


def _loopy_long(kind):
    if kind == "sis":
        N, T = 5, 20
        A = np.zeros((N, N), dtype=int)
        for i in range(N):
            A[i, (i + 1) % N] = A[(i + 1) % N, i] = 1
        A[0, 2] = A[2, 0] = 1                                  # the chord
        phi = [[np.array([0.8, 0.2]) if t == 0 else np.ones(2) for t in range(T + 1)] for _ in range(N)]
        for (i, t, v) in ((1, 7, [0.1, 0.9]), (3, 13, [1.0, 0.0]), (4, 20, [0.3, 0.7])):
            phi[i][t] = np.array(v)
        w = [[M.SISFactor(0.25, 0.15, 0.02)] * (T + 1) for _ in range(N)]
        return M.mpbp(M.IndexedBiDiGraph(A), w, 2, T, phi=phi, max_bond=4)
    N, T, qs = 4, 6, [2, 3, 2, 3]
    A = np.zeros((N, N), dtype=int)
    for i in range(N):
        A[i, (i + 1) % N] = A[(i + 1) % N, i] = 1
    rng = np.random.default_rng(3)
    phi = [[rng.random(q) + 0.1 for _ in range(T + 1)] for q in qs]
    w = [[M.SISFactor(0.3, 0.2)] * (T + 1) if q == 2 else [M.SIRSFactor(0.3, 0.2, 0.1, 0.05)] * (T + 1) for q in qs]
    return M.mpbp(M.IndexedBiDiGraph(A), w, qs, T, phi=phi, max_bond=4)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["sis", "mixed"])
def test_transfer_on_loopy_graph_matches_numpy_forward_backward(kind):
    bp = _loopy_long(kind)
    assert int(np.prod(bp.qnode)) == (32 if kind == "sis" else 36)
    s = M.ExactSolver(bp, "auto" if kind == "sis" else "transfer")
    assert s.method == "transfer"
    logZ, marg, pair = _numpy_forward_backward(bp)
    d = abs(s.logZ - logZ)
    assert d < 1e-10, f"logZ: observed difference {d:.3e}"
    _close("marginals", _flat(s.marginals()), _flat(marg))
    _close("pair marginals", _flat(s.pair_marginals()), _flat(pair))


# ------------------------------------------------------------------------------------------------ 6. MPBP against the truth
@pytest.mark.gpu
def test_mpbp_on_a_tree_matches_transfer_solver_at_T10():
    """SIS on a 5-node tree at T = 10: the messages are exact when nothing is truncated away (threshold 1e-14, and a bond
    capacity the run never reaches), so beliefs, pair beliefs and exp(-F_Bethe) are those of the exact solver"""
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
    s = M.ExactSolver(bp, "transfer")
    _close("beliefs", _flat(M.beliefs(bp)), _flat(s.marginals()), 1e-8)
    _close("pair beliefs", _flat(M.pair_beliefs(bp)[0]), _flat(s.pair_marginals()), 1e-8)
    _close("Z", np.exp(-M.bethe_free_energy(bp)), s.Z, 1e-8)


# ------------------------------------------------------------------------------------------------ 7. determinism
@pytest.mark.gpu
@pytest.mark.parametrize("method", ["enumerate", "transfer"])
def test_two_solves_are_bit_identical(method):
    bp = _case("a")[0]
    runs = []
    for _ in range(2):
        s = M.ExactSolver(bp, method)
        out = [np.array([s.logZ]), _flat(s.marginals()), _flat(s.pair_marginals())]
        if method == "enumerate":
            out.append(s.prob().ravel())
        runs.append(out)
    for a, b in zip(*runs):
        assert np.array_equal(a, b)


# ------------------------------------------------------------------------------------------------ 8. refusals
def _small_solve_still_works(bp):
    s = M.ExactSolver(bp, "auto")
    m = _flat(s.marginals())
    assert np.isfinite(s.logZ) and np.isfinite(m).all()


@pytest.mark.gpu
def test_refusals_leave_the_context_usable():
    sis = lambda N, T: M.mpbp(M.IndexedBiDiGraph(np.diag(np.ones(N - 1), 1) + np.diag(np.ones(N - 1), -1)),
                              [[M.SISFactor(0.3, 0.2)] * (T + 1)] * N, 2, T, max_bond=2)
    # Q over the limit: 2^42 configurations
    bp = sis(6, 6)
    with pytest.raises(M.MPBPError) as ei:
        M.ExactSolver(bp, "enumerate")
    assert ei.value.code == -4 and "2^32" in str(ei.value)
    _small_solve_still_works(bp)                                   # auto: transfer, S = 64
    # S over the limit: 17 binary nodes, refused at create
    bp = sis(17, 1)
    with pytest.raises(M.MPBPError) as ei:
        M.ExactSolver(bp, "transfer")
    assert ei.value.code == -4 and "2^16" in str(ei.value)
    M.iterate(bp, maxiter=1, svd_trunc=M.TruncBond(2))
    # periodic + transfer
    bp = _case("d")[0]
    with pytest.raises(M.MPBPError) as ei:
        M.ExactSolver(bp, "transfer")
    assert ei.value.code == -4 and "periodic" in str(ei.value)
    _small_solve_still_works(bp)
    # an aliased graph
    T = 2
    bp = M.mpbp_infinite_graph(3, [M.SISFactor(0.3, 0.2)] * (T + 1), 2, max_bond=4)
    for method in ("auto", "enumerate", "transfer"):
        with pytest.raises(M.MPBPError) as ei:
            M.ExactSolver(bp, method)
        assert ei.value.code == -4 and "aliased" in str(ei.value)
    M.iterate(bp, maxiter=1, svd_trunc=M.TruncBond(4))
    # prob(), site and edge trajectory marginals on a transfer solver name method 0
    bp = _case("a")[0]
    s = M.ExactSolver(bp, "transfer")
    for call in (s.prob, s.site_marginals, s.edge_marginals, s.alternate_marginals, s.autocorrelations):
        with pytest.raises(M.MPBPError) as ei:
            call()
        assert ei.value.code == -4 and "method 0" in str(ei.value)
    assert np.isfinite(s.logZ)
    _small_solve_still_works(bp)


@pytest.mark.gpu
def test_zero_partition_function_is_an_error_not_nans():
    """observations that exclude every trajectory (SIS without self-infection: all susceptible at t = 0, one node seen
    infectious at t = 1): MPBP_EINVAL from both methods, and the context stays usable"""
    T = 2
    phi = [[np.array([1.0, 0.0]) if t == 0 else np.ones(2) for t in range(T + 1)] for _ in range(3)]
    phi[1][1] = np.array([0.0, 1.0])
    bp = M.mpbp(M.IndexedBiDiGraph(PATH3), [[M.SISFactor(0.3, 0.2)] * (T + 1)] * 3, 2, T, phi=phi, max_bond=4)
    for method in ("enumerate", "transfer"):
        with pytest.raises(M.MPBPError) as ei:
            M.ExactSolver(bp, method).logZ
        assert ei.value.code == -1 and "Z = 0" in str(ei.value)
    M.reset_observations(bp)
    _small_solve_still_works(bp)
