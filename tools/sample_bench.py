"""Rate of the SoftMargin sampler (mpbp_sampler_*, csrc/sampler.hip): one JSON line with samples/s and us/sample on
  - the BASELINE configs[1] graph (SIS lambda=0.1 rho=0.05 gamma=0.1, networkx.random_regular_graph(3, 1024, seed=0), T=50),
    free, with observations drawn by draw_node_observations, and with two-time accumulation on 16 sites;
  - the karate club at T=200 (SIS, node 0 infected at t=0, as BASELINE configs[3]);
  - a vectorised numpy restatement of the configs[1] draw on one core, for scale.
Usage: python tools/sample_bench.py [--min-seconds 2]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import mpbp_amd as M  # noqa: E402


def rate(bp, min_seconds, **kw):
    """samples/s of M.sample on one sampler, doubling the call size until one call lasts min_seconds"""
    sms = M.SoftMarginSampler(bp, seed=1, **kw)
    M.sample(sms, 1024)                       # warm-up: tables, first launches
    n = 4096
    while True:
        t0 = time.perf_counter()
        M.sample(sms, n)
        dt = time.perf_counter() - t0
        if dt >= min_seconds or n >= 1 << 26:
            return n / dt, n, M.effective_sample_size(sms) / sms.nsamples
        n *= 2


def numpy_rate(A, T, lam, rho, gam, nsamp=64):
    """the configs[1] draw restated in numpy (vectorised over samples and nodes, one core): SIS transition of a 3-regular
    graph, x' = I with prob 1 - rho if infectious, else 1 - prod_k (1 - lam [x_k = I])"""
    rng = np.random.default_rng(0)
    N = A.shape[0]
    nbr = np.array([np.nonzero(A[i])[0] for i in range(N)])
    t0 = time.perf_counter()
    x = (rng.random((nsamp, N)) < gam).astype(np.int8)
    for _ in range(T):
        inf_nb = x[:, nbr]                                         # [S, N, 3]
        p_stay_s = np.prod(1 - lam * inf_nb, axis=2)
        p_inf = np.where(x == 1, 1 - rho, 1 - p_stay_s)
        x = (rng.random((nsamp, N)) < p_inf).astype(np.int8)
    return nsamp / (time.perf_counter() - t0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--min-seconds", type=float, default=2.0)
    a = ap.parse_args()
    import networkx as nx
    N, T, lam, rho, gam = 1024, 50, 0.1, 0.05, 0.1
    A = nx.to_numpy_array(nx.random_regular_graph(3, N, seed=0), nodelist=range(N))
    phi = [[np.array([1 - gam, gam]) if t == 0 else np.ones(2) for t in range(T + 1)] for _ in range(N)]
    bp = M.mpbp(M.IndexedBiDiGraph(A), [[M.SISFactor(lam, rho)] * (T + 1)] * N, 2, T, phi=phi, max_bond=4)
    out = {"tool": "sample_bench", "config1": "SIS 3-regular N=1024 T=50"}
    r, n, _ = rate(bp, a.min_seconds)
    out["config1_free_samples_per_s"], out["config1_free_us_per_sample"], out["config1_free_n"] = r, 1e6 / r, n
    r, n, _ = rate(bp, a.min_seconds, autocorr_sites=list(range(16)))
    out["config1_corr16_samples_per_s"], out["config1_corr16_us_per_sample"] = r, 1e6 / r
    bpo = M.mpbp(M.IndexedBiDiGraph(A), [[M.SISFactor(lam, rho)] * (T + 1)] * N, 2, T, phi=phi, max_bond=4)
    M.draw_node_observations(bpo, 64, softinf=1e2, rng=np.random.default_rng(0))
    r, n, ess = rate(bpo, a.min_seconds)
    out["config1_obs64_samples_per_s"], out["config1_obs64_us_per_sample"], out["config1_obs64_ess_fraction"] = r, 1e6 / r, ess
    K = np.loadtxt(os.path.join(ROOT, "tests", "golden", "karate.txt"))
    Nk, Tk = K.shape[0], 200
    phik = [[np.array([0.0, 1.0]) if (t == 0 and i == 0) else (np.array([1.0, 0.0]) if t == 0 else np.ones(2))
             for t in range(Tk + 1)] for i in range(Nk)]
    bpk = M.mpbp(M.IndexedBiDiGraph(K), [[M.SISFactor(0.1, 0.05)] * (Tk + 1)] * Nk, 2, Tk, phi=phik, max_bond=4)
    r, n, _ = rate(bpk, a.min_seconds)
    out["karate_T200_samples_per_s"], out["karate_T200_us_per_sample"] = r, 1e6 / r
    r = numpy_rate(A, T, lam, rho, gam)
    out["numpy_config1_samples_per_s"], out["numpy_config1_us_per_sample"] = r, 1e6 / r
    out["speedup_vs_numpy"] = out["config1_free_samples_per_s"] / r
    print(json.dumps(out))


if __name__ == "__main__":
    main()
