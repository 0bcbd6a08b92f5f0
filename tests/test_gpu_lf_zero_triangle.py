"""The engine skips the structural zeros of the triangular gauge factor Lf (csrc/engine.h, lf_zero / z_zero): Y1 does not write the
tiles of Z that lie wholly in the zero set, Y2 does not read the k-steps that hold nothing else and takes 0.0 for every element of
the set, M_t starts its contraction at the first chunk that is not all zero.  The rule under test: no lane ever uses a Z value of the zero set,
written or not.  MPBP_DEBUG_POISON_Z=1 fills the Z region of every slot with NaN before each engine launch, and the graphs here
are small enough (fewer problems per launch than slots) for every problem to see it: a lane that broke the rule turns the beliefs
into NaN.  Every case is driven through the public sweep API against the numpy oracle, sweep by sweep, at the tolerance of the
neighbouring parity tests (tests/test_gpu_parity.py, RTOL = 1e-6)."""
import functools

import networkx as nx
import numpy as np
import pytest

import mpbp_amd as M
from oracle import factors as OF
from oracle import mpbp as O
from oracle import tensor_trains as OT

RTOL = 1e-6
gpu = pytest.mark.gpu

SWITCHES = {
    "default": {},
    "v512": {"MPBP_DEBUG_NO_SMALL": "1"},
    "v64": {"MPBP_DEBUG_FORCE_SMALL": "1"},
    "grid": {"MPBP_GAUGE": "grid", "MPBP_DEBUG_NO_SMALL": "1"},       # sweep 1 batched: the EXT form of M_t
}


def _flat(bb):
    return np.array([p for b in bb for p in b])


def _rel(a, b):
    a, b = np.asarray(a, float), np.asarray(b, float)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


def _phi(N, T, p1):
    return [[np.array([1 - p1, p1]) if t == 0 else np.ones(2) for t in range(T + 1)] for _ in range(N)]


def _glauber_graph():
    G = nx.gnp_random_graph(8, 3 / 7, seed=2)
    return nx.to_numpy_array(G, nodelist=range(8))


# name -> (model, N, T, truncation, its argument, device bond capacity, sweeps)
CASES = {
    "sis_b3": ("sis", 8, 5, "TruncBond", 3, 3, 3),
    "sis_b5": ("sis", 8, 5, "TruncBond", 5, 5, 3),
    "glauber_b12": ("glauber", 8, 6, "TruncBond", 12, 12, 2),
    "sis_thresh": ("sis", 8, 6, "TruncThresh", 1e-6, 16, 3),
    "sis_b6": ("sis", 8, 6, "TruncBond", 6, 6, 3),
}


def _build(name, mod):
    """the model of a case on the device (mod = M) or in the oracle (mod = O)"""
    model, N, T, _, _, cap, _ = CASES[name]
    if model == "sis":
        lam, rho, gam = 0.15, 0.1, 0.2
        A = nx.to_numpy_array(nx.random_regular_graph(3, N, seed=0))
        phi = _phi(N, T, gam)
        if mod is M:
            return M.mpbp(M.IndexedBiDiGraph(A), [[M.SISFactor(lam, rho)] * (T + 1)] * N, 2, T, phi=phi, max_bond=cap)
        return O.mpbp(O.IndexedBiDiGraph(A), [[OF.SISFactor(lam, rho)] * (T + 1)] * N, [2] * N, T, phi=phi)
    A = _glauber_graph()
    J, h, phi = 0.5 * A, np.zeros(N), _phi(N, T, 0.2)
    if mod is M:
        return M.Glauber(M.Ising(J, h, 1.0), T, phi=phi).mpbp(max_bond=cap)
    return O.mpbp(O.IndexedBiDiGraph(A), OF.glauber_factors(A != 0, J, h, 1.0, T), [2] * N, T, phi=phi)


def _marginals(cores):
    return np.array(OT.marginals(OT.TensorTrain([np.array(a) for a in cores])))


@functools.lru_cache(maxsize=None)
def _oracle(name):
    """beliefs after every sweep, and the per-time marginals and bond table of every message after the last one"""
    _, _, _, trunc, arg, _, sweeps = CASES[name]
    obp = _build(name, O)
    bel = []
    for _ in range(sweeps):
        O.iterate(obp, maxiter=1, svd_trunc=getattr(OT, trunc)(arg), tol=0.0, shuffle_nodes=False, jacobi=True)
        bel.append(_flat(O.beliefs(obp)))
    for b in bel:
        b.setflags(write=False)
    return bel, [_marginals(m.tensors) for m in obp.mu], np.array([m.bonds for m in obp.mu])


def _device(name, switches, monkeypatch, poison=True):
    for k, v in SWITCHES[switches].items():
        monkeypatch.setenv(k, v)
    if poison:
        monkeypatch.setenv("MPBP_DEBUG_POISON_Z", "1")
    _, _, _, trunc, arg, _, sweeps = CASES[name]
    bp = _build(name, M)
    bel = []
    for _ in range(sweeps):
        M.iterate(bp, maxiter=1, svd_trunc=getattr(M, trunc)(arg), tol=0.0)
        st = bp.last_stats
        assert st.nan_flag == 0 and st.jacobi_not_converged == 0 and st.capacity_flag == 0
        bel.append(_flat(M.beliefs(bp)))
    return bp, bel


def _check(name, switches, monkeypatch):
    obel, omarg, obonds = _oracle(name)
    bp, bel = _device(name, switches, monkeypatch)
    for s, (b, ob) in enumerate(zip(bel, obel)):
        assert np.isfinite(b).all(), f"sweep {s}"
        assert _rel(b, ob) < RTOL, f"sweep {s}"
    assert np.array_equal(bp.bonds(), obonds)
    for e, cores in enumerate(bp.get_messages()):
        m = _marginals(cores)
        assert np.isfinite(m).all() and _rel(m, omarg[e]) < RTOL, f"edge {e}"


def test_cases_truncate_in_the_oracle():
    """Every case must have binding truncation (else r1 = Bn everywhere and little of the zero triangle is exercised) and a
    finite oracle result; the Glauber graph must hold degree-3 nodes, whose cavity products have ny1 != ny2, and one of degree
    >= 4, where a product of three neighbours (ny1 = 4) at bond 12 contracts over bn * ny1 = 48 > 40 indices."""
    degs = dict(nx.from_numpy_array(_glauber_graph()).degree()).values()
    assert 3 in degs and max(degs) >= 4
    for name, (_, N, T, trunc, arg, cap, _) in CASES.items():
        bel, marg, bonds = _oracle(name)
        assert all(np.isfinite(b).all() for b in bel) and all(np.isfinite(m).all() for m in marg), name
        full = np.array([1] + [min(4 ** t, 4 ** (T + 1 - t)) for t in range(1, T + 1)] + [1])     # ranks without truncation
        assert (bonds < full[None, :]).any(), name
        if trunc == "TruncBond":
            assert bonds.max() == arg, name                   # a bond reaches its cap
        else:
            assert 1 < bonds.max() <= cap, name               # data-dependent ranks inside the device capacity


@gpu
@pytest.mark.parametrize("switches", ["default", "v512", "v64"])
@pytest.mark.parametrize("name", ["sis_b3", "sis_b5"])
def test_sis_poisoned_z_matches_oracle(name, switches, monkeypatch):
    """Bonds that are no multiple of 4 or 16, r1 of 9 to 25, an != bn while the bonds still grow (first sweep) and saturated
    steps after it, on the 512-thread and on the single-wave build."""
    _check(name, switches, monkeypatch)


@gpu
@pytest.mark.parametrize("switches", ["default", "v512"])
def test_glauber_degree3_poisoned_z_matches_oracle(switches, monkeypatch):
    """ny1 != ny2 along the cavity of the degree-3 node, and bn * ny1 > 40 at bond 12: the general path of gemm_direct, not the
    one with cached index maps."""
    _check("glauber_b12", switches, monkeypatch)


@gpu
def test_trunc_thresh_poisoned_z_matches_oracle(monkeypatch):
    """Data-dependent ranks: r1 < Bn in the middle of the chain (trapezoidal Lf)."""
    _check("sis_thresh", "v512", monkeypatch)


@gpu
def test_grid_gauge_poisoned_z_matches_oracle(monkeypatch):
    """Lf from the batched gauge sweep (k_lf_write): the EXT form of the engine, where only the M_t part applies."""
    _check("sis_b6", "grid", monkeypatch)


@gpu
def test_second_run_is_bit_identical(monkeypatch):
    """Without the poison: the same case twice in one process.  The second run finds the first one's numbers in the Z tiles that
    Y1 no longer writes; were any of them used, the two runs would differ."""
    runs = []
    for _ in range(2):
        bp, bel = _device("sis_b3", "default", monkeypatch, poison=False)
        runs.append((bel, bp.bonds(), [np.concatenate([a.ravel() for a in c]) for c in bp.get_messages()]))
    (b1, d1, m1), (b2, d2, m2) = runs
    assert all(np.array_equal(x, y) for x, y in zip(b1, b2))
    assert np.array_equal(d1, d2)
    assert all(np.array_equal(x, y) for x, y in zip(m1, m2))
