"""bench.py --dump-outputs: the per-time message marginals it writes, the files of one small run, and --steps."""
import itertools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_message_marginals_match_enumeration():
    import bench
    import mpbp_amd as M
    T = 4
    cores = M.random_message(T, 2, 5, np.random.default_rng(3))
    m = bench._message_marginals(cores)
    full = np.zeros((4,) * (T + 1))
    for cfg in itertools.product(range(4), repeat=T + 1):
        v = np.ones((1, 1))
        for t, c in enumerate(cfg):
            v = v @ cores[t][:, :, c // 2, c % 2]
        full[cfg] = v[0, 0]
    full /= full.sum()
    for t in range(T + 1):
        ref = full.sum(axis=tuple(s for s in range(T + 1) if s != t)).reshape(2, 2)
        np.testing.assert_allclose(m[t], ref, rtol=1e-12, atol=1e-15)


def test_bench_rejects_zero_steps():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "0"], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 2 and "--steps" in r.stderr


@pytest.mark.gpu
def test_bench_dump_outputs(tmp_path):
    """One small run: the dumped beliefs / f are the ones --dump-beliefs writes, every file is float64, the whole dump
    stays under 64 MB, and the JSON line reports the requested number of timed steps."""
    out = tmp_path / "out"
    one = str(tmp_path / "one.npy")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--nodes", "32", "--T", "8", "--bond", "6",
                        "--steps", "3", "--warmup", "1", "--no-cpu-baseline", "--dump-beliefs", one,
                        "--dump-outputs", str(out)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    j = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    assert j["steps"] == 3 and len(j["device_ms_steps"]) == 3
    d = {k: np.load(out / f"{k}.npy") for k in ("beliefs", "free_energy", "bonds", "message_marginals", "message_edges")}
    assert all(v.dtype == np.float64 for v in d.values())
    assert sum(v.nbytes for v in d.values()) <= 64 << 20
    ref = np.load(one, allow_pickle=True).item()
    assert np.array_equal(d["beliefs"], ref["beliefs"]) and np.array_equal(d["free_energy"], ref["f"])
    assert d["beliefs"].shape == (32, 9, 2) and d["bonds"].shape == (96, 10)
    assert d["message_marginals"].shape == (d["message_edges"].size, 9, 2, 2)
    np.testing.assert_allclose(d["message_marginals"].sum(axis=(2, 3)), 1.0, rtol=1e-12)
