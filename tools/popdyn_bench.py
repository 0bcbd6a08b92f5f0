"""Rate of the population dynamics sweep (mpbp_popdyn_*, csrc/popdyn.hip): one JSON line with member updates per second
for popsize 2^16, 2^20 and 2^24 on
  - RandomRegular(3): pkm1 = Dirac(2), two gathers per member, no table look-up;
  - ErdosRenyi(3.0):  pkm1 = Poisson(3), three gathers per member on average, one cdf scan;
pJ = Dirac(1), ph = Dirac(0), beta = 1.  Each figure is `--sweeps` sweeps in one mpbp_popdyn_iterate call (queued on the
device, one synchronisation at the end) after `--warmup` sweeps, the median of `--repeats` such calls.
Usage: python tools/popdyn_bench.py [--sweeps 50] [--warmup 5] [--repeats 3]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import mpbp_amd as M  # noqa: E402
from mpbp_amd import equilibrium as E  # noqa: E402


def rate(pkm1, popsize, sweeps, warmup, repeats):
    """member updates per second of `sweeps` queued sweeps; the means are not copied out (a NULL mean_after_each)"""
    pop = M.PopDyn(np.random.default_rng(0).standard_normal(popsize), beta=1.0, seed=1)
    for which, d in ((E.PKM1, pkm1), (E.PK, pkm1), (E.PJ, M.Dirac(1.0)), (E.PH, M.Dirac(0.0))):
        pop.set_distribution(which, d)
    L = M._lib.lib()
    M._lib.check(L.mpbp_popdyn_iterate(pop._h, warmup, None))
    times = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        M._lib.check(L.mpbp_popdyn_iterate(pop._h, sweeps, None))      # returns after the device has finished
        times.append(time.perf_counter() - t0)
    assert np.all(np.isfinite(pop.get_population()))
    dt = float(np.median(times))
    return popsize * sweeps / dt, dt / sweeps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sweeps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=3)
    a = ap.parse_args()
    out = {"tool": "popdyn_bench", "sweeps": a.sweeps, "warmup": a.warmup, "repeats": a.repeats}
    for name, pkm1, gathers in (("rr3", M.Dirac(2), 2.0), ("er3", M.Poisson(3.0), 3.0)):
        out[f"{name}_gathers_per_member"] = gathers
        for lg in (16, 20, 24):
            r, per_sweep = rate(pkm1, 1 << lg, a.sweeps, a.warmup, a.repeats)
            out[f"{name}_2^{lg}_updates_per_s"] = r
            out[f"{name}_2^{lg}_us_per_sweep"] = 1e6 * per_sweep
    print(json.dumps(out))


if __name__ == "__main__":
    main()
