"""Time pigs_vh_accumulate for Ntau = 0, 8, 16 beside pigs_grv_accumulate with Nbin = 16 in the same process, at config
3's shape (Np 256, 161 beads, 128 walkers, window 20, Nr = Ns = 100, random in-box worldlines).  The figure of merit is
the time per pair visit relative to pigs_grv_accumulate's: the van Hove kernel visits Np^2 ordered pairs per slice pair
and sum_l (2 window + 1 - l) slice pairs per walker, k_grv Np (Np - 1) / 2 pairs per window slice.

Host wall clock over `--calls` queued calls closed by one read (which synchronises), after a warm-up of the same shape,
best of `--repeats` and median.  Prints one JSON line and writes it to --out when given.

  python scripts/vh_bench.py [--window 20] [--calls 10] [--repeats 5] [--ntau 0 8 16] [--form -1] [--out profiles/vh_bench.json]
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
    ap.add_argument("--np", type=int, default=256, dest="Np")
    ap.add_argument("--ntau", type=int, nargs="+", default=[0, 8, 16])
    ap.add_argument("--bins", type=int, default=100)
    ap.add_argument("--form", type=int, nargs="+", default=[-1])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert api.device_count() >= 1, "needs a GPU"
    cfg = SystemConfig(dim=3, Np=a.Np, Nb=80, density=0.365)
    VT, WF = api.build_tables(cfg)
    W = a.walkers
    P = np.random.default_rng(1982).uniform(-0.5, 0.5, (W,) + tuple(cfg.path_shape)) * np.asarray(cfg.Lbox[:3])
    ns = 2 * a.window + 1
    grv_pairs = float(cfg.Np * (cfg.Np - 1) // 2) * ns * W
    res = {"Np": cfg.Np, "beads": cfg.path_shape[0], "walkers": W, "window": a.window, "calls": a.calls, "Nr": a.bins,
           "Ns": a.bins, "vh": []}
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
        res["grv_nbin16"] = {"ms_per_call_min": gbest * 1e3, "ms_per_call_median": gmed * 1e3, "pair_visits_per_call": grv_pairs,
                             "ns_per_pair_visit": gbest * 1e9 / grv_pairs}
        for form in a.form:
            ctx.set_tuning("vh_form", form)
            for ntau in a.ntau:
                visits = float(cfg.Np) ** 2 * sum(ns - l for l in range(ntau + 1)) * W
                ctx.vh_init(ntau, a.window, a.bins, cfg.rcut / a.bins, a.bins, cfg.rcut / a.bins)
                best, med = timed(ctx.vh_accumulate, lambda: ctx.vh_read(reset=True))
                res["vh"].append({"form": form, "Ntau": ntau, "ms_per_call_min": best * 1e3, "ms_per_call_median": med * 1e3,
                                  "pair_visits_per_call": visits, "ns_per_pair_visit": best * 1e9 / visits,
                                  "per_visit_ratio_to_grv": (best / visits) / (gbest / grv_pairs)})
        ctx.set_tuning("vh_form", -1)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
