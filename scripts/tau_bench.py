"""Time pigs_tau_accumulate against pigs_therm_energy_batch -- existing code that visits the same
pairs on 160 of the same 161 slices -- at config 3's shape (Np 256, 161 beads, 128 walkers, jittered-lattice worldlines),
in one process and one context, the legs interleaved.

Host wall clock over `--calls` calls (pigs_tau_accumulate: queued, closed by one read, which synchronises;
pigs_therm_energy_batch synchronises itself), after a warm-up of the same shape; per leg the median, minimum and maximum
over `--repeats`.  The acceptance rule of DESIGN.md: the tau median lies within the therm median plus that leg's own
max - min spread.  Prints one JSON line.

  python scripts/tau_bench.py [--calls 10] [--repeats 7] [--walkers 128]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pathintegralgroundstate_amd import SystemConfig, api  # noqa: E402


def lattice(cfg, W, rng):
    n = int(np.ceil(cfg.Np ** (1.0 / cfg.dim) - 1e-9))
    L = np.asarray(cfg.Lbox[:cfg.dim])
    idx = np.stack(np.unravel_index(np.arange(cfg.Np), (n,) * cfg.dim), axis=1).astype(float)
    return (idx[None, None] + 0.5 + rng.uniform(-0.1, 0.1, (W,) + tuple(cfg.path_shape))) * (L / n) - 0.5 * L


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--walkers", type=int, default=128)
    a = ap.parse_args()
    assert api.device_count() >= 1, "needs a GPU"
    cfg = SystemConfig(dim=3, Np=256, Nb=80, density=0.365)
    VT, WF = api.build_tables(cfg)
    W = a.walkers
    P = lattice(cfg, W, np.random.default_rng(1982))
    res = {"Np": cfg.Np, "beads": cfg.path_shape[0], "walkers": W, "calls": a.calls, "repeats": a.repeats}
    with api.PigsContext(cfg, VT, WF, n_walkers=W) as ctx:
        ctx.upload_all(P)
        ctx.tau_init()

        def tau():
            for _ in range(a.calls):
                ctx.tau_accumulate()
            ctx.tau_read(reset=True)

        def therm():
            for _ in range(a.calls):
                ctx.therm_energy_batch()

        legs = {"tau_accumulate": tau, "therm_energy_batch": therm}
        t = {k: [] for k in legs}
        for k, f in legs.items():
            f()                                             # warm-up of this shape
        for _ in range(a.repeats):
            for k, f in legs.items():
                t0 = time.perf_counter()
                f()
                t[k].append((time.perf_counter() - t0) / a.calls * 1e3)
        for k, v in t.items():
            v = sorted(v)
            res[k] = {"ms_per_call_median": v[len(v) // 2], "ms_per_call_min": v[0], "ms_per_call_max": v[-1]}
    y, x = res["therm_energy_batch"], res["tau_accumulate"]
    limit = y["ms_per_call_median"] + (y["ms_per_call_max"] - y["ms_per_call_min"])
    x["ratio_to_therm_median"] = x["ms_per_call_median"] / y["ms_per_call_median"]
    x["within_therm_spread"] = bool(x["ms_per_call_median"] <= limit)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
