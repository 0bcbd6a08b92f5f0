"""Wall time of the exact solvers (mpbp_exact_*, csrc/exact.hip): one JSON line with the seconds of `solve` plus all
marginals and pair marginals for
  - joint enumeration at Q = 2^30: SIS on the 5-node path, T = 5;
  - global-state transfer at S = 2^12, T = 50: SIS on networkx.random_regular_graph(3, 12, seed=0);
  - global-state transfer at S = 2^16, T = 50: the same on 16 nodes;
and the seconds of `twovar_marginals` over all nodes plus `alternate_twovar_marginals` (maxdist = 10, the forward-backward
pass they start with included) on the same two transfer models, T = 50: cases tt12 and tt16.  A vector-step is one
conditioned vector through one transfer matrix, 2 S^2 flop: sum_i q_i (sum_t min(maxdist, T - t) + T) of them.  The tt cases
report the seconds per vector-step, and - when the tr case of the same S ran too - its ratio to the solver's single-vector
step (seconds / 2T), and the fraction of the fp64 MFMA peak (78.6 Tflop/s) that the vector-steps' flops amount to.
Each case is run `--repeat` times on a fresh solver after one warm-up; the minimum is reported.
Usage: python tools/exact_bench.py [--repeat 2] [--cases enum30,tr12,tr16,tt12,tt16]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import mpbp_amd as M  # noqa: E402


def sis(A, T, lam=0.1, rho=0.05, gam=0.1):
    N = A.shape[0]
    phi = [[np.array([1 - gam, gam]) if t == 0 else np.ones(2) for t in range(T + 1)] for _ in range(N)]
    return M.mpbp(M.IndexedBiDiGraph(A), [[M.SISFactor(lam, rho)] * (T + 1)] * N, 2, T, phi=phi, max_bond=2)


def seconds(bp, method, repeat):
    """min over `repeat` fresh solvers of solve + marginals + pair marginals (after one warm-up solver)"""
    best, logZ = float("inf"), None
    for k in range(repeat + 1):
        t0 = time.perf_counter()
        s = M.ExactSolver(bp, method)
        logZ = s.logZ
        s.marginals()
        s.pair_marginals()
        dt = time.perf_counter() - t0
        del s
        if k > 0:
            best = min(best, dt)
    return best, logZ


def twotime_seconds(bp, maxdist, repeat):
    """min over `repeat` fresh transfer solvers of twovar_marginals (all nodes) + alternate_twovar_marginals"""
    best = float("inf")
    for k in range(repeat + 1):
        s = M.ExactSolver(bp, "transfer")
        t0 = time.perf_counter()
        s.twovar_marginals(maxdist=maxdist)
        s.alternate_twovar_marginals()
        dt = time.perf_counter() - t0
        del s
        if k > 0:
            best = min(best, dt)
    return best


FP64_MFMA_PEAK = 78.6e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=2)
    ap.add_argument("--cases", default="enum30,tr12,tr16,tt12,tt16")
    a = ap.parse_args()
    import networkx as nx
    out = {"tool": "exact_bench"}
    cases = a.cases.split(",")
    if "enum30" in cases:
        N = 5
        A = np.diag(np.ones(N - 1), 1) + np.diag(np.ones(N - 1), -1)
        out["enumerate_Q2^30_path5_T5_seconds"], out["enumerate_Q2^30_logZ"] = seconds(sis(A, 5), "enumerate", a.repeat)
    for key, N in (("tr12", 12), ("tr16", 16)):
        if key in cases:
            A = nx.to_numpy_array(nx.random_regular_graph(3, N, seed=0), nodelist=range(N))
            out[f"transfer_S2^{N}_T50_seconds"], out[f"transfer_S2^{N}_logZ"] = seconds(sis(A, 50), "transfer", a.repeat)
    T, md = 50, 10
    for key, N in (("tt12", 12), ("tt16", 16)):
        if key in cases:
            A = nx.to_numpy_array(nx.random_regular_graph(3, N, seed=0), nodelist=range(N))
            sec = twotime_seconds(sis(A, T), md, a.repeat)
            steps = 2 * N * (sum(min(md, T - t) for t in range(T)) + T)
            pre = f"twotime_S2^{N}_T{T}_maxdist{md}"
            out[pre + "_seconds"], out[pre + "_vector_steps"] = sec, steps
            out[pre + "_seconds_per_vector_step"] = sec / steps
            out[pre + "_fp64_mfma_peak_fraction"] = steps * 2.0 * (2.0 ** N) ** 2 / sec / FP64_MFMA_PEAK
            single = out.get(f"transfer_S2^{N}_T50_seconds")
            if single is not None:
                out[pre + "_vector_step_over_single_vector_step"] = (sec / steps) / (single / (2 * T))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
