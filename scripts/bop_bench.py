"""Time pigs_bop_accumulate without and with the correlation pass (Nr = 0, Nr = 100) beside pigs_grv_accumulate with
Nbin = 16 in the same process -- the same pair count -- at config 3's shape (Np 256, 161 beads, 128 walkers, window 20,
random in-box worldlines, the neighbour radius that holds about 12 particles).

Host wall clock over `--calls` queued calls closed by one read (which synchronises), after a warm-up of the same shape,
best of `--repeats` and median.  Prints one JSON line and writes it to --out when given.

  python scripts/bop_bench.py [--window 20] [--calls 10] [--repeats 5] [--nr 0 100] [--out profiles/bop_bench.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pathintegralgroundstate_amd import SystemConfig, api  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=int, default=20)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--walkers", type=int, default=128)
    ap.add_argument("--nr", type=int, nargs="+", default=[0, 100])
    ap.add_argument("--neighbours", type=float, default=12.0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert api.device_count() >= 1, "needs a GPU"
    cfg = SystemConfig(dim=3, Np=256, Nb=80, density=0.365)
    VT, WF = api.build_tables(cfg)
    W = a.walkers
    P = np.random.default_rng(1982).uniform(-0.5, 0.5, (W,) + tuple(cfg.path_shape)) * np.asarray(cfg.Lbox[:3])
    ns = 2 * a.window + 1
    pairs = float(cfg.Np * (cfg.Np - 1) // 2) * ns * W
    rnb = (3.0 * a.neighbours / (4.0 * np.pi * cfg.density)) ** (1.0 / 3.0)
    res = {"Np": cfg.Np, "beads": cfg.path_shape[0], "walkers": W, "window": a.window, "calls": a.calls, "rnb": rnb,
           "pairs_per_call": pairs, "bop": []}
    with api.PigsContext(cfg, VT, WF, n_walkers=W) as ctx:
        ctx.upload_all(P)

        def timed(acc, read):
            acc()
            read()                                          # warm-up of this shape
            t = []
            for _ in range(a.repeats):
                t0 = time.perf_counter()
                for _ in range(a.calls):
                    acc()
                read()
                t.append((time.perf_counter() - t0) / a.calls)
            return min(t), sorted(t)[len(t) // 2]

        ctx.grv_init(16, a.window)
        gbest, gmed = timed(ctx.grv_accumulate, lambda: ctx.grv_read(reset=True))
        res["grv_nbin16"] = {"ms_per_call_min": gbest * 1e3, "ms_per_call_median": gmed * 1e3, "pairs_per_s": pairs / gbest}
        for nr in a.nr:
            ctx.bop_init(rnb, a.window, 50, nr, cfg.rcut / nr if nr else None)
            best, med = timed(ctx.bop_accumulate, lambda: ctx.bop_read(reset=True))
            ctx.bop_accumulate()
            got = ctx.bop_read(reset=True)
            res["bop"].append({"Nr": nr, "ms_per_call_min": best * 1e3, "ms_per_call_median": med * 1e3,
                               "pairs_per_s": pairs / best, "ratio_to_grv": best / gbest,
                               "coordination": float(got["S"][:, 6].sum() / (W * ns * cfg.Np))})
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
