"""Time pigs_sqv_accumulate against pigs_fqt_accumulate, the only other code that evaluates density harmonics over a
window, at config 3's shape (Np 256, 161 beads, 128 walkers, random in-box worldlines).

Host wall clock over `--calls` queued calls closed by one read (which synchronises), after a warm-up of the same shape.
Prints one JSON line: ms per call and ns per (harmonic, particle, slice) term of each, and their ratio.

  python scripts/sqv_bench.py [--nmax 8] [--window 20] [--nk 50] [--calls 10] [--repeats 5] [--only sqv|fqt]
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
    ap.add_argument("--nmax", type=int, default=8)
    ap.add_argument("--window", type=int, default=20)
    ap.add_argument("--nk", type=int, default=50)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--walkers", type=int, default=128)
    ap.add_argument("--only", choices=["sqv", "fqt"], default=None)
    a = ap.parse_args()
    assert api.device_count() >= 1, "needs a GPU"
    cfg = SystemConfig(dim=3, Np=256, Nb=80, density=0.365)
    VT, WF = api.build_tables(cfg)
    W = a.walkers
    P = np.random.default_rng(1982).uniform(-0.5, 0.5, (W,) + tuple(cfg.path_shape)) * np.asarray(cfg.Lbox[:3])
    ns = 2 * a.window + 1
    res = {"Np": cfg.Np, "beads": cfg.path_shape[0], "walkers": W, "window": a.window, "calls": a.calls}
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

        if a.only in (None, "sqv"):
            ctx.sqv_init(a.nmax, a.window)
            nq = ctx.sqv_vectors().shape[0]
            best, med = timed(ctx.sqv_accumulate, ctx.sqv_read)
            terms = float(nq) * cfg.Np * ns * W
            res["sqv"] = {"nmax": a.nmax, "harmonics": nq, "ms_per_call_min": best * 1e3, "ms_per_call_median": med * 1e3,
                          "ns_per_term": best * 1e9 / terms, "terms_per_call": terms}
        if a.only in (None, "fqt"):
            ctx.fqt_init(a.nk, 0, a.window)
            best, med = timed(ctx.fqt_accumulate, ctx.fqt_read)
            terms = float(a.nk * 3) * cfg.Np * ns * W
            res["fqt"] = {"Nk": a.nk, "harmonics": a.nk * 3, "ms_per_call_min": best * 1e3, "ms_per_call_median": med * 1e3,
                          "ns_per_term": best * 1e9 / terms, "terms_per_call": terms}
    if "sqv" in res and "fqt" in res:
        res["cost_per_term_sqv_over_fqt"] = res["sqv"]["ns_per_term"] / res["fqt"]["ns_per_term"]
    print(json.dumps(res))


if __name__ == "__main__":
    main()
