"""Time pigs_fqs_accumulate (the self part of F(q,tau) and the displacement) next to pigs_fqv_accumulate at the same shape:
config 3's (Np 256, 161 beads, 128 walkers, random in-box worldlines), nmax 4 and 8, window 20, all 41 lags.

Host wall clock over `--calls` queued calls closed by one read (which synchronises), after a warm-up of the same shape:
best of `--repeats`, with the median.  Prints one JSON line and, with --out, writes it (profiles/fqs_bench.json).

  python scripts/fqs_bench.py [--nmax 4 8] [--window 20] [--ntau 40] [--calls 3] [--repeats 3] [--out FILE]
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
    ap.add_argument("--nmax", type=int, nargs="+", default=[4, 8])
    ap.add_argument("--window", type=int, default=20)
    ap.add_argument("--ntau", type=int, default=40)
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--walkers", type=int, default=128)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert api.device_count() >= 1, "needs a GPU"
    cfg = SystemConfig(dim=3, Np=256, Nb=80, density=0.365)
    VT, WF = api.build_tables(cfg)
    W = a.walkers
    P = np.random.default_rng(1982).uniform(-0.5, 0.5, (W,) + tuple(cfg.path_shape)) * np.asarray(cfg.Lbox[:3])
    ns = 2 * a.window + 1
    pairs = sum(ns - l for l in range(a.ntau + 1))
    res = {"Np": cfg.Np, "beads": cfg.path_shape[0], "walkers": W, "window": a.window, "ntau": a.ntau, "calls": a.calls}
    with api.PigsContext(cfg, VT, WF, n_walkers=W) as ctx:
        ctx.upload_all(P)

        def timed(acc, read):
            acc()
            read(reset=True)                                # warm-up of this shape
            t = []
            for _ in range(a.repeats):
                t0 = time.perf_counter()
                for _ in range(a.calls):
                    acc()
                read(reset=True)
                t.append((time.perf_counter() - t0) / a.calls)
            return min(t), sorted(t)[len(t) // 2]

        for nmax in a.nmax:
            ctx.fqs_init(nmax, a.ntau, a.window)
            nq = ctx.fqs_vectors().shape[0]
            sb, sm = timed(ctx.fqs_accumulate, ctx.fqs_read)
            ctx.fqs_init(1, 0, 0)                           # give the accumulators back
            ctx.fqv_init(nmax, a.ntau, a.window)
            vb, vm = timed(ctx.fqv_accumulate, ctx.fqv_read)
            ctx.fqv_init(1, 0, 0)
            res[f"nmax{nmax}"] = {"vectors": nq,
                                  "fqs_ms_per_call_min": sb * 1e3, "fqs_ms_per_call_median": sm * 1e3,
                                  "fqv_ms_per_call_min": vb * 1e3, "fqv_ms_per_call_median": vm * 1e3,
                                  "fqs_over_fqv": sb / vb,
                                  "fqs_lag_terms_per_call": float(nq) * cfg.Np * W * pairs,
                                  "fqv_lag_terms_per_call": float(nq) * W * pairs}
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
