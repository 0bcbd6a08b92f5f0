#!/usr/bin/env python3
"""Benchmark of the MPBP message-update hot path (BASELINE.json metric: edge-message updates/sec and
s/sweep, SIS on a 3-regular random graph, N=1024, T=50, max bond 20 = BASELINE configs[1]).

A "step" is one Jacobi sweep of onebpiter! over all nodes (E = 3072 edge-message updates), messages
resident in HBM.  Usage:  python bench.py --gpus N --steps K --warmup W
For N > 1 launch with  python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N ...
(one rank per GPU over RCCL; nodes are sharded, one all-gather of the message slots per sweep).
Rank 0 prints ONE JSON line."""
import argparse
import json
import os
import sys
import time

os.environ.setdefault("OPENBLAS_NUM_THREADS", "1")
os.environ.setdefault("OMP_NUM_THREADS", "1")
ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

FP64_PEAK_TFLOPS = 78.6         # MI355X fp64 matrix (= vector) peak, public spec; BASELINE.md section 2
FP32_MFMA_PEAK_TFLOPS = 157.3   # fp32 matrix peak (north_star asks for this fraction too)
HBM_PEAK_TBPS = 8.0             # HBM3E spec (about 6.3 TB/s achievable, MI355X_MICROARCH.md)


# ------------------------------------------------------------------------------------------------
# CPU baseline: the numpy oracle (a port of the reference algorithm: LAPACK gesdd SVD sweeps) timed on
# a bounded sample of the same workload.  Only this leg imports oracle/.
# ------------------------------------------------------------------------------------------------
def _cpu_heavy_op(args):
    os.environ["OPENBLAS_NUM_THREADS"] = "1"
    lam, rho, T, Mb, b1, b2 = args
    from oracle import mpbp as O
    from oracle.factors import SISFactor
    from oracle.tensor_trains import TensorTrain, TruncBond
    wi = [SISFactor(lam, rho)] * (T + 1)
    t0 = time.perf_counter()
    O.op_kron_compress(wi, (TensorTrain(b1), 1), (TensorTrain(b2), 1), T, TruncBond(Mb))
    return time.perf_counter() - t0


def _cpu_heavy_op_qr(args):
    os.environ["OPENBLAS_NUM_THREADS"] = "1"
    lam, rho, T, Mb, b1, b2 = args
    from oracle.device_algorithm import op_kron_compress_qr
    from oracle.factors import SISFactor
    from oracle.tensor_trains import TensorTrain, TruncBond
    wi = [SISFactor(lam, rho)] * (T + 1)
    t0 = time.perf_counter()
    op_kron_compress_qr(wi, (TensorTrain(b1), 1), (TensorTrain(b2), 1), T, TruncBond(Mb))
    return time.perf_counter() - t0


def _cpu_model():
    try:
        for ln in open("/proc/cpuinfo"):
            if ln.startswith("model name"):
                return ln.split(":", 1)[1].strip()
    except OSError:
        pass
    return "unknown"


def _host_cores():
    """CPUs this process may really use: the scheduler affinity, capped by the cgroup CPU quota (a one-GPU box of the
    pool is a 16-CPU share of a 256-thread host: 256 workers there just time-slice 16 CPUs)."""
    n = len(os.sched_getaffinity(0))
    why = "sched_getaffinity"
    try:
        q, per = open("/sys/fs/cgroup/cpu.max").read().split()[:2]
        if q != "max":
            c = max(1, int(round(int(q) / int(per))))
            if c < n:
                n, why = c, "cgroup cpu.max"
    except (OSError, ValueError):
        try:
            q = int(open("/sys/fs/cgroup/cpu/cpu.cfs_quota_us").read())
            per = int(open("/sys/fs/cgroup/cpu/cpu.cfs_period_us").read())
            if q > 0 and max(1, round(q / per)) < n:
                n, why = max(1, round(q / per)), "cgroup cfs quota"
        except (OSError, ValueError):
            pass
    env = os.environ.get("MPBP_BENCH_CPU_CORES")
    if env:
        n, why = int(env), "MPBP_BENCH_CPU_CORES"
    return n, why


def cpu_baseline(node_msgs, lam, rho, gam, T, Mb, E_per_sweep, n_heavy=64):
    """node_msgs: the incoming messages (lists of cores) of several degree-3 nodes from the device state after the
    warm-up sweeps.  Sample: >= n_heavy heavy `op`s (Kronecker 20x20 -> compress!, 100 SVDs up
    to 400x1600) drawn from those nodes' message pairs, one process per host core (all of os.sched_getaffinity);
    on one core the cheap parts (one light `op` with `init`, one message finalisation, the belief).  A degree-3 node
    update = 4 heavy + 3 light ops + 3 finalisations + 1 belief (cavity order, reference
    src/recursive_bp_factor.jl:140 with CavityTools.cavity)."""
    import multiprocessing as mp
    from oracle import mpbp as O
    from oracle.factors import SISFactor
    from oracle.tensor_trains import TensorTrain, TruncBond, compress, normalize, normalize_eachmatrix
    cores, cores_why = _host_cores()
    wi = [SISFactor(lam, rho)] * (T + 1)
    psi = [np.ones((2, 2))] * (T + 1)
    phi = [np.array([1 - gam, gam]) if t == 0 else np.ones(2) for t in range(T + 1)]
    pairs = []
    for msgs3 in node_msgs:
        B = [O.prob_xy_apply(wi, 2, TensorTrain(m), psi, k, T) for k, m in enumerate(msgs3)]
        for (i, j) in ((0, 1), (1, 2), (0, 2)):
            pairs.append(([c.copy() for c in B[i][0].tensors], [c.copy() for c in B[j][0].tensors]))
    n_ops = max(n_heavy, cores)
    n_ops = ((n_ops + cores - 1) // cores) * cores          # whole rounds: every core busy for the whole sample
    jobs = [(lam, rho, T, Mb) + pairs[k % len(pairs)] for k in range(n_ops)]
    t0 = time.perf_counter()
    with mp.get_context("spawn").Pool(cores) as pool:
        th = pool.map(_cpu_heavy_op, jobs, chunksize=1)
        wall = time.perf_counter() - t0
        # second, stronger baseline: the DEVICE's algorithm (R-only QR gauge sweep + SVD of the small factor,
        # oracle/device_algorithm.py) on the same host cores - one round of the same operand pairs
        thq = pool.map(_cpu_heavy_op_qr, jobs[:cores], chunksize=1)
    t_heavy = float(np.mean(th))
    t_heavy_qr = float(np.mean(thq))
    tr = TruncBond(Mb)
    B = [O.prob_xy_apply(wi, 2, TensorTrain(m), psi, k, T) for k, m in enumerate(node_msgs[0])]
    a = O.op_kron_compress(wi, B[0], B[1], T, tr)
    init = O.init_train(wi, 2, T)
    t0 = time.perf_counter()
    dest = O.op_kron_compress(wi, a, init, T, tr)
    t_light = time.perf_counter() - t0
    t0 = time.perf_counter()
    Bm = O.f_bp_partial_ij(dest[0], wi, phi, 2, 2, 1)
    mu = compress(O.mpem2(Bm), tr, is_orthogonal="left")
    normalize_eachmatrix(mu)
    normalize(mu)
    t_fin = time.perf_counter() - t0
    t0 = time.perf_counter()
    full = dest      # any bond-saturated ỹ-train: the belief step costs the same
    bb = O.marginalize(O.mpem2(O.f_bp_partial_i(full[0], wi, phi, 3)))
    normalize(bb)
    t_bel = time.perf_counter() - t0
    t_node = 4 * t_heavy + 3 * t_light + 3 * t_fin + t_bel
    rate = cores * 3.0 / t_node
    t_node_qr = 4 * t_heavy_qr + 3 * t_light + 3 * t_fin + t_bel
    return {"value": rate, "unit": "edge-updates/s", "cores": cores, "kind": "port", "cpu_model": _cpu_model(),
            "nproc": os.cpu_count(), "cores_from": cores_why, "s_per_sweep": E_per_sweep / rate, "n_heavy_ops_sampled": n_ops,
            "sample_wall_s": wall,
            "device_algorithm_on_cpu": {"value": cores * 3.0 / t_node_qr, "unit": "edge-updates/s", "kind": "port",
                                        "s_per_heavy_op": t_heavy_qr,
                                        "sample": f"{cores} heavy ops with the device's algorithm (LAPACK geqrf R-only gauge sweep + gesdd of "
                                                  f"M_t, oracle/device_algorithm.py), one per core: {t_heavy_qr:.2f} s per op against "
                                                  f"{t_heavy:.2f} s for the reference algorithm"},
            "sample": (f"numpy oracle (LAPACK gesdd), {n_ops} heavy ops from the message pairs of {len(node_msgs)} nodes on "
                       f"{cores} processes (all CPUs this process may use: {cores_why}; mean {t_heavy:.2f} s per op per core, {wall:.0f} s wall) + "
                       f"light op {t_light:.3f} s + finalisation {t_fin:.3f} s + belief {t_bel:.3f} s on the "
                       f"post-warm-up messages; node update = 4 heavy + 3 light + 3 fin + 1 belief "
                       f"= {t_node:.1f} s/core")}


def _cpu_short_op(args):
    """Seconds of the reference-algorithm `op` (Kronecker + compress!, LAPACK gesdd sweeps) on two random trains of Lc and
    of Lc + 1 cores whose bonds all sit at the cap Mb - the steady-state time steps of a saturated chain, without the chain.
    Returns (t(Lc), t(Lc + 1))."""
    kind, Mb, Lc, d1, d2, threads, seed = args
    os.environ["OPENBLAS_NUM_THREADS"] = str(threads)
    from oracle import mpbp as O
    from oracle import factors as OF
    from oracle.tensor_trains import TensorTrain, TruncBond
    rng = np.random.default_rng(seed)
    w = OF.HomogeneousGlauberFactor(0.5, 0.0, 1.0) if kind == "glauber" else OF.SISFactor(0.1, 0.05)

    def run(L_, bond):
        mk = lambda d: TensorTrain([rng.uniform(0.5, 1.5, size=(bond, bond, w.nstates(d), 2)) / (bond * 4) for _ in range(L_)])   # noqa: E731
        a, b = (mk(d1), d1), (mk(d2), d2)
        t0 = time.perf_counter()
        O.op_kron_compress([w] * L_, a, b, L_ - 1, TruncBond(bond))
        return time.perf_counter() - t0
    run(Lc, min(Mb, 6))          # first-call costs (imports, BLAS start-up)
    t_a = run(Lc, Mb)
    if t_a < 5.0:
        t_a = run(Lc, Mb)        # cheap enough to repeat: the first full-size run also pays the page faults of its work arrays
    return t_a, run(Lc + 1, Mb)


def cpu_baseline_big(config, T, Mb, deg, nstates, E_per_sweep):
    """configs[2..4]: a whole reference-algorithm `op` at these bond caps takes minutes to hours on a CPU core, so the sample
    is the STEADY-STATE TIME STEPS of one: the `op` on chains of Lc and Lc + 1 cores with every bond (ends included) at the cap;
    the difference is one saturated time step (both SVD sweeps + Kronecker build + carry).  That time prices
    SURVEY 8(d)'s reference flop count of the same step (flops.op_flops), and the resulting flop rate of the reference
    algorithm on this host prices the whole sweep (flops.node_update_flops over the config's degrees).  configs[2], [3]:
    one process per host core on independent operands; configs[4] has ONE message: one process, BLAS threads = cores."""
    import multiprocessing as mp
    from mpbp_amd import flops as F
    cores, cores_why = _host_cores()
    kind = "glauber" if config == 2 else "sis"
    d1 = d2 = 2 if config == 2 else 1                   # a product from the middle of a Glauber cavity (nstates 3 x 3 -> 5)
    par = 1 if config == 4 else cores
    thr = cores if config == 4 else 1
    Lc = 2
    jobs = [(kind, Mb, Lc, d1, d2, thr, 100 + k) for k in range(par)]
    t0 = time.perf_counter()
    with mp.get_context("spawn").Pool(par) as pool:
        th = pool.map(_cpu_short_op, jobs, chunksize=1)
    wall = time.perf_counter() - t0
    t_short, t_long = float(np.mean([x[0] for x in th])), float(np.mean([x[1] for x in th]))
    t_step = max(t_long - t_short, 1e-9)
    ny = (lambda l: l + 1) if config == 2 else (lambda l: 1 if l == 0 else 2)

    def ref_flops(L_):          # SURVEY 8(d)'s count on a chain with bond-1 ends, long enough to saturate in the middle
        b = [min(Mb, 4 ** min(t, L_ - t)) if min(t, L_ - t) < 16 else Mb for t in range(L_ + 1)]
        return F.op_flops(b, b, b, ny(d1), ny(d2), ny(d1 + d2), 2)[1]
    step_flops = ref_flops(61) - ref_flops(60)                     # one saturated time step
    rate = step_flops / t_step                                      # reference-algorithm flop/s of one process
    L = T + 1
    prof = [min(Mb, 4 ** min(t, L - t)) if min(t, L - t) < 16 else Mb for t in range(L + 1)]
    tot = 0.0
    for z in sorted(set(int(d) for d in deg)):
        if z > 0:
            tot += F.node_update_flops(prof, z, 2, ny)["reference_total"] * int(np.sum(np.asarray(deg) == z))
    s_per_sweep = tot / (rate * par)
    return {"value": E_per_sweep / s_per_sweep, "unit": "edge-updates/s", "cores": cores, "kind": "port", "cpu_model": _cpu_model(),
            "cores_from": cores_why, "s_per_sweep": s_per_sweep, "sample_wall_s": wall,
            "reference_flops_per_sweep": tot, "reference_flop_rate_per_process": rate, "s_per_saturated_time_step": t_step,
            "sample": (f"numpy oracle (LAPACK gesdd): reference-algorithm `op` at bond cap {Mb} ({kind}, nstates {ny(d1)} x {ny(d2)} -> "
                       f"{ny(d1 + d2)}) on chains of {Lc} and {Lc + 1} cores with every bond at the cap, {par} process(es) x {thr} BLAS "
                       f"thread(s) ({cores_why}): {t_short:.1f} s and {t_long:.1f} s -> {t_step:.1f} s per saturated time step = "
                       f"{rate / 1e9:.1f} Gflop/s of SURVEY 8(d)'s count per process; the sweep = {tot / 1e12:.1f} Tflop of that count "
                       f"(flops.node_update_flops over the config's degrees, T = {T}) -> {s_per_sweep:.0f} s per sweep")}


DUMP_MAX_BYTES = 64 << 20      # --dump-outputs: at most 64 MB in all
DUMP_EDGE_SAMPLE = 64          # messages sampled for --dump-outputs (fixed seed)


def _message_marginals(cores):
    """[T+1, q, q] per-time marginals of one message (MPEM2 cores [b_t, b_{t+1}, q, q]): the function the message
    represents, summed over every other time step.  Gauge free, unlike the cores, so two builds compare entry by entry."""
    S = [a.sum(axis=(2, 3)) for a in cores]
    left = [np.ones(1)]
    for s in S[:-1]:
        v = left[-1] @ s
        left.append(v / np.abs(v).max())
    right = [np.ones(1)]
    for s in S[:0:-1]:
        v = s @ right[-1]
        right.append(v / np.abs(v).max())
    right = right[::-1]
    out = np.empty((len(cores),) + cores[0].shape[2:])
    for t, a in enumerate(cores):
        m = np.einsum("a,abxy,b->xy", left[t], a, right[t])
        out[t] = m / m.sum()
    return out


def dump_outputs(path, bp, parts):
    """--dump-outputs: what the timed path computed in its last step, as float64 .npy files under `path` - beliefs and
    free-energy terms of the nodes the step updated (`parts`: (lo, hi, beliefs, f) per node block), the bond table of
    every edge, and the per-time marginals of a seeded sample of the messages the step wrote (their edge ids beside)."""
    os.makedirs(path, exist_ok=True)
    ptr, _, oute = bp.g.nbr_arrays()
    written = np.unique(np.concatenate([np.asarray(oute[int(ptr[lo]):int(ptr[hi])]) for lo, hi, _, _ in parts]))
    rng = np.random.default_rng(0)
    edges = np.sort(rng.choice(written, size=min(DUMP_EDGE_SAMPLE, written.size), replace=False))
    marg = []
    for k in range(0, edges.size, 16):                 # a few messages per download: bounded host memory
        chunk = edges[k:k + 16]
        msgs = bp.get_messages(edges=chunk)
        marg += [_message_marginals(msgs[int(e)]) for e in chunk]
    out = {"beliefs": np.concatenate([p_[2] for p_ in parts]),
           "free_energy": np.concatenate([p_[3] for p_ in parts]),
           "bonds": bp.bonds(),
           "message_marginals": np.stack(marg),
           "message_edges": edges}
    out = {k: np.ascontiguousarray(v, dtype=np.float64) for k, v in out.items()}
    total = sum(v.nbytes for v in out.values())
    if total > DUMP_MAX_BYTES:
        raise SystemExit(f"--dump-outputs: {total} bytes exceed the {DUMP_MAX_BYTES}-byte limit")
    for k, v in out.items():
        np.save(os.path.join(path, k + ".npy"), v)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--config", type=int, default=1, choices=[1, 2, 3, 4],
                    help="index into BASELINE.json configs: 1 = SIS 3-regular N=1024 T=50 d=20 (the metric's config, default), "
                         "2 = Glauber ER N=2048 T=100 d=30, 3 = SIS karate T=200 d=40, 4 = infinite graph k=3 T=200 d=64")
    ap.add_argument("--nodes", type=int, default=0, help="override the number of nodes (configs 1, 2)")
    ap.add_argument("--T", type=int, default=0, help="override the chain length")
    ap.add_argument("--bond", type=int, default=0, help="override the bond cap")
    ap.add_argument("--shard-of", type=int, default=0,
                    help="with one process: run only rank 0's node block of a K-way sharding (what one GPU of K does per sweep)")
    ap.add_argument("--shard-index", type=int, default=0, help="with --shard-of K: which rank's node block to run (default 0)")
    ap.add_argument("--cpu-sample", type=int, default=64, help="heavy ops timed by the CPU baseline (>= host cores)")
    ap.add_argument("--saturate", action="store_true",
                    help="start from random normalised messages at the saturated bond profile on the in-edges of the owned "
                         "nodes (the dimensions of a converged state without the sweeps that lead there; use with --warmup 0)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--backend", default="nccl", help="torch.distributed backend for N>1 (gloo = rehearsal on one GPU)")
    ap.add_argument("--dump-beliefs", default="", help="write rank-0 beliefs + f to this .npy file (parity checks)")
    ap.add_argument("--dump-outputs", default="", metavar="DIR",
                    help="after the timed steps write what the last one computed as float64 .npy files under DIR "
                         "(beliefs, free-energy terms, bond table, per-time marginals of a seeded sample of messages)")
    ap.add_argument("--phase-profile", action="store_true", help="print the engine phase profile to stderr")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")
    if args.warmup < 0:
        ap.error("--warmup must not be negative")

    import torch
    import torch.distributed as dist
    import networkx as nx
    import mpbp_amd as M
    from mpbp_amd import dist as D
    from mpbp_amd import flops as F

    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        if rank == 0:
            print(f"warning: --gpus {args.gpus} but WORLD_SIZE={world}; using WORLD_SIZE", file=sys.stderr)
    ndev = torch.cuda.device_count()
    if world > max(ndev, 1):
        # rehearsal with several ranks on one GPU: the cooperative panel kernel of the batched gauge sweep assumes that its
        # workgroups are co-resident, i.e. that the process owns the device (include/mpbp_hip.h) - use the per-column launches
        os.environ["MPBP_DEBUG_NO_COOP_PANEL"] = "1"
    local = local % max(ndev, 1)          # rehearsal: several ranks may share one GPU (gloo backend)
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if args.backend == "nccl":
            dist.init_process_group("nccl", device_id=dev)
        else:
            dist.init_process_group(args.backend)

    # ---- workload: inputs of the chosen BASELINE config
    dflt = {1: (1024, 50, 20), 2: (2048, 100, 30), 3: (34, 200, 40), 4: (1, 200, 64)}[args.config]
    N, T, Mb = args.nodes or dflt[0], args.T or dflt[1], args.bond or dflt[2]
    lam, rho, gam = 0.1, 0.05, 0.1
    nstates = lambda l: 1 if l == 0 else 2          # SIS (sis_bp.jl:18)
    shardable = args.config in (1, 2)
    if args.config == 1:
        G = nx.random_regular_graph(3, N, seed=0)
        A = nx.to_numpy_array(G, nodelist=range(N))
        facs = [[M.SISFactor(lam, rho)] * (T + 1)] * N
        phi = [[np.array([1 - gam, gam]) if t == 0 else np.ones(2) for t in range(T + 1)] for _ in range(N)]
        wl = (f"SIS lambda=0.1 rho=0.05 gamma=0.1 on networkx.random_regular_graph(3,{N},seed=0), T={T}, TruncBond({Mb}), "
              f"Jacobi sweeps (BASELINE configs[1])")
    elif args.config == 2:
        G = nx.gnp_random_graph(N, 4 / (N - 1), seed=0)
        A = nx.to_numpy_array(G, nodelist=range(N))
        m0 = -0.6
        facs = M.glauber_factors(A != 0, 0.5 * A, np.zeros(N), 1.0, T)
        phi = [[np.array([(1 + m0) / 2, (1 - m0) / 2]) if t == 0 else np.ones(2) for t in range(T + 1)] for _ in range(N)]
        nstates = lambda l: l + 1                   # HomogeneousGlauberFactor (glauber_bp.jl:32)
        wl = (f"homogeneous Glauber J=0.5 h=0 beta=1, m0=-0.6 on networkx.gnp_random_graph({N},4/{N - 1},seed=0), T={T}, "
              f"TruncBond({Mb}), Jacobi sweeps (BASELINE configs[2])")
    elif args.config == 3:
        A = np.loadtxt(os.path.join(ROOT, "tests", "golden", "karate.txt"))
        N = A.shape[0]
        lam, rho = 0.1, 0.05
        facs = [[M.SISFactor(lam, rho)] * (T + 1)] * N
        phi = [[np.array([0.0, 1.0]) if (t == 0 and i == 0) else (np.array([1.0, 0.0]) if t == 0 else np.ones(2))
                for t in range(T + 1)] for i in range(N)]
        wl = f"SIS lambda=0.1 rho=0.05, node 0 infected at t=0, karate club (34 nodes, degrees 1..17), T={T}, TruncBond({Mb}) (BASELINE configs[3])"
    else:
        A = None
        lam, rho = 0.1, 0.2
        wl = f"infinite-graph fixed point (src/infinite_graph.jl), SIS lambda=0.1 rho=0.2 gamma=0.1, k=3, T={T}, TruncBond({Mb}) (BASELINE configs[4])"
    if A is not None:
        g = M.IndexedBiDiGraph(A)
        E = g.ne()
        ptr, ine, oute = g.nbr_arrays()
        deg = np.diff(np.asarray(ptr))
        nshard = world if shardable else 1
        if world == 1 and args.shard_of > 1 and shardable:
            nshard = args.shard_of
        # shards are cut by predicted time: the executed flops of a rank's nodes at the measured rate + the part of its deepest
        # node's dependency chain that runs alone on the chip (dist.node_times / shard_nodes_by_time)
        work_s, tail_s = D.node_times(ptr, 2, Mb, T, nstates=nstates)
        if shardable and world > 1:
            slot, S, shards = D.slot_map(ptr, oute, E, world, shards=D.shard_nodes_by_time(ptr, world, work_s, tail_s))
            nslots = world * S
        else:
            slot, S, nslots = np.arange(E, dtype=np.int32), E, E
            shards = D.shard_nodes_by_time(ptr, nshard, work_s, tail_s) if nshard > 1 else [(0, N)]
        if shardable and (world > 1 or nshard > 1):
            # fails here, before any allocation, if a rank cannot hold slab + snapshot + its largest node (dist.memory_plan)
            D.memory_plan(ptr, 2, Mb, T, shards, nstates=nstates, hbm_bytes=float(torch.cuda.get_device_properties(dev).total_memory))
        slot_doubles = (T + 1) * Mb * Mb * 4
        cores_t = torch.zeros(nslots, slot_doubles, dtype=torch.float64, device=dev)
        bonds_t = torch.zeros(nslots, T + 2, dtype=torch.int32, device=dev)
        bp = M.mpbp(g, facs, 2, T, phi=phi, max_bond=Mb, device=local, slot_of_edge=slot,
                    n_slots=nslots, ext_cores=cores_t.data_ptr(), ext_bonds=bonds_t.data_ptr())
        if not (0 <= args.shard_index < len(shards)):
            raise SystemExit(f"--shard-index {args.shard_index} out of range for {len(shards)} shards")
        lo, hi = shards[rank if (shardable and world > 1) else (args.shard_index if (world == 1 and args.shard_of > 1 and shardable) else 0)]
    else:
        phi1 = [np.array([1 - gam, gam]) if t == 0 else np.ones(2) for t in range(T + 1)]
        bp = M.mpbp_infinite_graph(3, [M.SISFactor(lam, rho)] * (T + 1), 2, phi1, max_bond=Mb, device=local)
        E, deg, lo, hi, ptr, ine = 3, np.array([3]), 0, 1, [0, 3], None
        cores_t = bonds_t = None
    exchange = shardable and world > 1
    if args.saturate and A is not None:
        rng = np.random.default_rng(1234 + rank + args.shard_index)
        msgs = [None] * E
        for i in range(lo, hi):
            for p_ in range(int(ptr[i]), int(ptr[i + 1])):
                msgs[int(ine[p_])] = M.random_message(T, 2, Mb, rng)
        bp.set_messages(msgs)
        del msgs
    # heartbeat on stderr: a long silent run looks hung to the job runner
    import threading
    t_start = time.time()

    def _beat():
        while True:
            time.sleep(60)
            print(f"[bench] running, {time.time() - t_start:.0f} s", file=sys.stderr, flush=True)
    threading.Thread(target=_beat, daemon=True).start()
    bp._L.mpbp_set_profiling(bp._h, 2 if args.phase_profile else 1)
    owned = np.arange(lo, hi, dtype=np.int32)
    trunc = M.TruncBond(Mb)
    ms_orth, n_orth, ms_dev, ms_xchg = [], [], [], []

    def step(record):
        M.onebpiter(bp, owned, trunc)
        if record:
            st = bp.last_stats
            ms_orth.append(st.ms_orth); n_orth.append(st.n_orth_launches); ms_dev.append(st.ms_total)
        if exchange:
            # mpbp_sweep returned after a stream synchronise: everything from here to the next synchronise is the exchange
            # (including the wait for the slowest rank: the collective cannot complete before every rank has entered it)
            t_x = time.perf_counter()
            D.allgather_slots(cores_t, bonds_t, S, rank, world)
            torch.cuda.synchronize()
            if record:
                ms_xchg.append((time.perf_counter() - t_x) * 1e3)

    def fence():
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()

    for _ in range(args.warmup):
        step(False)
    fence()
    import ctypes as C
    ph = np.zeros(24)
    bp._L.mpbp_phase_profile(bp._h, ph.ctypes.data_as(C.POINTER(C.c_double)), 24, 1)
    t0 = time.perf_counter()
    for _ in range(args.steps):
        step(True)
    fence()
    dt = time.perf_counter() - t0
    if world > 1:
        tt = torch.tensor([dt], dtype=torch.float64, device=dev if args.backend == "nccl" else "cpu")
        dist.all_reduce(tt, op=dist.ReduceOp.MAX)
        dt = float(tt.item())

    if args.dump_beliefs or args.dump_outputs:
        # beliefs / f of the nodes this rank owns; rank 0 gathers them
        b = np.array(M.beliefs(bp))[lo:hi]
        f = np.zeros(N)
        bp._L.mpbp_free_energy(bp._h, f.ctypes.data_as(C.POINTER(C.c_double)))
        if world > 1:
            parts = [None] * world
            dist.all_gather_object(parts, (lo, hi, b, f[lo:hi]))
        else:
            parts = [(lo, hi, b, f[lo:hi])]
        if rank == 0 and args.dump_beliefs:
            ball = np.concatenate([p_[2] for p_ in parts]); fall = np.concatenate([p_[3] for p_ in parts])
            np.save(args.dump_beliefs, {"beliefs": ball, "f": fall}, allow_pickle=True)
        if rank == 0 and args.dump_outputs:
            dump_outputs(args.dump_outputs, bp, parts)
    if rank == 0 and args.phase_profile:
        bp._L.mpbp_phase_profile(bp._h, ph.ctypes.data_as(C.POINTER(C.c_double)), 24, 0)
        names = ["stage", "Y1", "Y2", "qr1_panel", "qr1_trail", "Lf", "N", "Mt", "qr2_panel", "qr2_trail", "jacobi",
                 "trunc", "carry", "norm"]
        tot = ph[:len(names)].sum()
        st = bp.last_stats
        print(f"jacobi: {st.jacobi_sweeps} sweeps in {st.jacobi_calls} calls (last sweep, all engine launches)", file=sys.stderr)
        print("engine phase profile (workgroup-seconds, cavity-op launches):", file=sys.stderr)
        for n_, v in zip(names, ph):
            print(f"  {n_:10s} {v:10.3f} s  {100 * v / max(tot, 1e-30):5.1f} %", file=sys.stderr)
    # per-rank split of a step, so that the first multi-GPU record can be read: the sweep of the rank's own node block
    # (device time of mpbp_sweep) and the exchange (all-gather + the wait for the slowest rank), means over the timed steps
    per_rank = None
    if world > 1:
        mine = (float(np.mean(ms_dev)) if ms_dev else 0.0, float(np.mean(ms_xchg)) if ms_xchg else 0.0)
        allr = [None] * world
        dist.all_gather_object(allr, mine)
        per_rank = {"sweep_ms": [a for a, _ in allr], "exchange_ms": [b for _, b in allr]}
    if rank == 0:
        ms_per_step = dt / args.steps * 1e3
        replicas = world > 1 and not shardable       # configs 3 / 4 do not shard by node: N independent replicas
        e_job = (int(ptr[hi]) - int(ptr[lo])) if (world == 1 and args.shard_of > 1 and shardable) else E * (world if replicas else 1)
        value = e_job * args.steps / dt
        # ---- roofline of the dominant kernel family (the cavity `op` launches: eng_kernel, and for the batched gauge
        #      sweep its grid kernels; HIP events on the library's stream around every such launch, rank 0)
        b = bp.bonds()
        prof = [int(v) for v in b.max(axis=0)]
        ex = refalg = 0.0
        for z in sorted(set(int(d) for d in deg[lo:hi])):
            if z == 0:
                continue
            fl = F.node_update_flops(prof, z, 2, nstates)
            cnt = int(np.sum(deg[lo:hi] == z))
            ex += fl["executed_ops"] * cnt * args.steps
            refalg += fl["reference_ops"] * cnt * args.steps
        launches = int(np.sum(n_orth))
        t_orth = float(np.sum(ms_orth)) * 1e-3
        achieved = ex / t_orth / 1e12 if t_orth > 0 else 0.0
        # HBM-side bytes per launch: rocprofv3 --pmc passes of this same command, committed under profiles/ (bench.py
        # cannot run the profiler on itself) - quoted, not measured in this run, and only for the configuration they
        # were taken on
        traffic, traffic_src = None, None
        for rnd in ("r04", "r03", "r02", "r01"):
            pmc = os.path.join(ROOT, "profiles", f"{rnd}_pmc_eng_kernel.json")
            if world == 1 and args.config == 1 and (N, T, Mb) == (1024, 50, 20) and os.path.exists(pmc):
                with open(pmc) as fh:
                    traffic = json.load(fh)["bytes_per_launch_avg"]
                traffic_src = f"profiles/{rnd}_pmc_eng_kernel.json (FETCH_SIZE x2 gfx950 correction + WRITE_SIZE, per launch; quoted from the committed profile, not measured in this run)"
                break
        avg_launch_s = (t_orth / launches) if launches else None
        roofline = {"bound": "mfma", "achieved": achieved, "peak": FP64_PEAK_TFLOPS, "unit": "TFLOP/s",
                    "frac": achieved / FP64_PEAK_TFLOPS, "frac_fp32_mfma": achieved / FP32_MFMA_PEAK_TFLOPS,
                    "traffic": traffic, "traffic_source": traffic_src,
                    "hbm_GBps": (traffic / avg_launch_s / 1e9) if (traffic and avg_launch_s) else None,
                    "frac_hbm": (traffic / avg_launch_s / 1e12 / HBM_PEAK_TBPS) if (traffic and avg_launch_s) else None,
                    "kernel": "cavity op launches (v512::eng_kernel; batched gauge sweep kernels when enabled)", "launches": launches,
                    "avg_launch_ms": (avg_launch_s * 1e3) if launches else None,
                    "flops_per_launch_executed": ex / launches if launches else None,
                    "achieved_reference_algorithmic": refalg / t_orth / 1e12 if t_orth > 0 else 0.0,
                    "frac_reference_algorithmic": (refalg / t_orth / 1e12 / FP64_PEAK_TFLOPS) if t_orth > 0 else 0.0,
                    "note": "achieved / frac count the flops the engine executes (structured contractions + R-only "
                            "Householder QR + Jacobi on the small factor) against the fp64 MFMA peak (78.6 TFLOP/s); "
                            "frac_fp32_mfma prices the same fp64 work against the fp32 matrix peak north_star names "
                            "(157.3 TFLOP/s); frac_hbm = memory-side bytes per launch / launch time / 8 TB/s; "
                            "*_reference_algorithmic price the launches with SURVEY.md 8(d)'s count for the reference "
                            "algorithm (SVD-based, 601.6 Gflop per node at configs[1]), which the device path "
                            "legitimately undercuts and which can therefore exceed the peak"}
        metric = ("edge-message updates/sec (and s/sweep), SIS 3-regular N=1024 T=50 d=20" if args.config == 1
                  else f"edge-message updates/sec (and s/sweep), BASELINE configs[{args.config}]")
        par = "1 GPU"
        if exchange:
            par = f"nodes sharded over {world} GPU(s) by predicted cost, 1 all-gather/sweep"
        elif replicas:
            par = f"{world} independent replicas (this config does not shard by node)"
        elif world == 1 and args.shard_of > 1 and shardable:
            par = f"rank {args.shard_index}'s node block [{lo},{hi}) of a {args.shard_of}-way sharding, on 1 GPU"
        out = {"metric": metric,
               "value": value, "unit": "edge-updates/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
               "ms_per_step": ms_per_step, "s_per_sweep": ms_per_step / 1e3, "higher_is_better": True,
               "scaling": "weak" if replicas else "strong", "vs_baseline": None, "dtype": "f64", "data": "synthetic",
               "config": {"workload": wl, "edges": int(E), "edge_updates_per_step": int(e_job), "parallelism": par,
                          "bond_profile_max": prof[:5] + ["..."] + prof[-4:]},
               "device_ms_per_step": float(np.mean(ms_dev)), "device_ms_steps": [float(v) for v in ms_dev], "roofline": roofline}
        if per_rank is not None:
            out["per_rank"] = per_rank
        free_b, tot_b = torch.cuda.mem_get_info(dev)
        out["hbm_in_use_GiB"] = (tot_b - free_b) / 2 ** 30
        if world == 1 and not args.no_cpu_baseline and args.config == 1:
            d3 = [i for i in range(lo, hi) if deg[i] == 3][:8]
            node_msgs = []
            for i in d3:
                e_in = [int(ine[p]) for p in range(ptr[i], ptr[i + 1])]
                msgs = bp.get_messages(edges=e_in)
                node_msgs.append([msgs[e] for e in e_in])
            out["cpu_baseline"] = cpu_baseline(node_msgs, lam, rho, gam, T, Mb, E, n_heavy=args.cpu_sample)
            out["speedup_vs_cpu_baseline"] = value / out["cpu_baseline"]["value"]
        elif world == 1 and not args.no_cpu_baseline:
            out["cpu_baseline"] = cpu_baseline_big(args.config, T, Mb, deg, nstates, E)
            # `value` counts the edge updates THIS run did (a node block under --shard-of), like the CPU figure per edge update
            out["speedup_vs_cpu_baseline"] = value / out["cpu_baseline"]["value"]
        print(json.dumps(out))
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
