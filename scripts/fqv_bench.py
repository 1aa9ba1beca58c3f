"""Time pigs_fqv_accumulate at Ntau = 0 and at all lags against pigs_sqv_accumulate, the existing code that does the same
phasor work, at config 3's shape (Np 256, 161 beads, 128 walkers, random in-box worldlines).

Host wall clock over `--calls` queued calls closed by one read (which synchronises), after a warm-up of the same shape:
best of `--repeats`, with the median.  Prints one JSON line.  The split between k_fqv_rho and k_fqv_correlate comes from
a kernel trace of `--only fqv` (profiles/fqv_kernel_stats.txt), not from this clock.

  python scripts/fqv_bench.py [--nmax 8] [--window 20] [--ntau 40] [--calls 10] [--repeats 5] [--only sqv|fqv] [--trace]

--trace is the shape of the kernel-trace run: fqv at --ntau only (no Ntau = 0 pass, so that every k_fqv_correlate call in
the trace has all the lags) and sqv, one repeat each.
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
    ap.add_argument("--ntau", type=int, default=40)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--walkers", type=int, default=128)
    ap.add_argument("--only", choices=["sqv", "fqv"], default=None)
    ap.add_argument("--trace", action="store_true")
    a = ap.parse_args()
    if a.trace:
        a.repeats = 1
    assert api.device_count() >= 1, "needs a GPU"
    cfg = SystemConfig(dim=3, Np=256, Nb=80, density=0.365)
    VT, WF = api.build_tables(cfg)
    W = a.walkers
    P = np.random.default_rng(1982).uniform(-0.5, 0.5, (W,) + tuple(cfg.path_shape)) * np.asarray(cfg.Lbox[:3])
    ns = 2 * a.window + 1
    res = {"Np": cfg.Np, "beads": cfg.path_shape[0], "walkers": W, "nmax": a.nmax, "window": a.window, "calls": a.calls}
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

        if a.only in (None, "fqv"):
            for ntau in sorted({a.ntau} if a.trace else {0, a.ntau}):
                ctx.fqv_init(a.nmax, ntau, a.window)
                nq = ctx.fqv_vectors().shape[0]
                best, med = timed(ctx.fqv_accumulate, ctx.fqv_read)
                lag_terms = float(nq) * W * sum(ns - l for l in range(ntau + 1))
                res[f"fqv_ntau{ntau}"] = {"vectors": nq, "ms_per_call_min": best * 1e3, "ms_per_call_median": med * 1e3,
                                          "phasor_terms_per_call": float(nq) * cfg.Np * ns * W, "lag_terms_per_call": lag_terms,
                                          "scratch_bytes": 16.0 * nq * ns * W}
        if a.only in (None, "sqv"):
            ctx.sqv_init(a.nmax, a.window)
            nq = ctx.sqv_vectors().shape[0]
            best, med = timed(ctx.sqv_accumulate, ctx.sqv_read)
            res["sqv"] = {"vectors": nq, "ms_per_call_min": best * 1e3, "ms_per_call_median": med * 1e3,
                          "phasor_terms_per_call": float(nq) * cfg.Np * ns * W}
    if "sqv" in res:
        for k in [k for k in res if k.startswith("fqv_")]:
            res[k]["ms_over_sqv"] = res[k]["ms_per_call_min"] / res["sqv"]["ms_per_call_min"]
    print(json.dumps(res))


if __name__ == "__main__":
    main()
