"""Time pigs_sf_accumulate beside pigs_fqs_accumulate (nmax 2; the same window and lags) on one context, at config 3's
shape (Np 256, 161 beads, 128 walkers, window 20, Ntau 20): random walks of 3 % of the box per link and axis, wrapped
into the cell.

Every call is timed by two events on the context's stream, after one warm-up call of the same shape; the figures are
medians (and minima) over --calls calls.  One context, no retries.  --resources takes the kernel resource figures (a JSON
object, from the gfx950 compile of pigs_sf.hip) into the result.  Prints one JSON line and writes it to --out when given.

Not measured here: the cost per MC step in a front-end run, 1D and 2D, shapes other than config 3's, other nmax of fqs.

  timeout 300 python scripts/sf_bench.py [--window 20] [--ntau 20] [--calls 5] [--out profiles/sf_bench.json]
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pathintegralgroundstate_amd import SystemConfig, api  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=int, default=20)
    ap.add_argument("--ntau", type=int, default=20)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--walkers", type=int, default=128)
    ap.add_argument("--np", type=int, default=256, dest="Np")
    ap.add_argument("--fqs-nmax", type=int, default=2)
    ap.add_argument("--resources", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    assert api.device_count() >= 1 and torch.cuda.is_available(), "needs a GPU"
    cfg = SystemConfig(dim=3, Np=a.Np, Nb=80, density=0.365)
    VT, WF = api.build_tables(cfg)
    W, L = a.walkers, np.asarray(cfg.Lbox[:3])
    rng = np.random.default_rng(1995)
    P = rng.uniform(-0.5, 0.5, (W, 1, a.Np, 3)) * L + np.cumsum(rng.normal(0.0, 0.03, (W,) + tuple(cfg.path_shape)) * L, axis=1)
    P = P - L * np.floor((P + 0.5 * L) / L)
    res = {"Np": cfg.Np, "beads": cfg.path_shape[0], "walkers": W, "window": a.window, "ntau": a.ntau, "calls": a.calls,
           "fqs_nmax": a.fqs_nmax}
    with api.PigsContext(cfg, VT, WF, n_walkers=W) as ctx:
        ctx.upload_all(P)
        ks = torch.cuda.ExternalStream(ctx.stream(), device=torch.device("cuda", torch.cuda.current_device()))

        def timed(acc):
            acc()
            ctx.sync()                                      # warm-up of this shape
            ms = []
            for _ in range(a.calls):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(ks)
                acc()
                e1.record(ks)
                e1.synchronize()
                ms.append(e0.elapsed_time(e1))
            return float(np.median(ms)), float(min(ms))

        ctx.fqs_init(a.fqs_nmax, a.ntau, a.window)
        fmed, fmin = timed(ctx.fqs_accumulate)
        res["fqs"] = {"ms_per_call_median": fmed, "ms_per_call_min": fmin}
        ctx.sf_init(a.ntau, a.window)
        ctx.sf_accumulate()
        got = ctx.sf_read(reset=True)
        assert got["samples"].tolist() == [1] * W and int(got["nwrap"].min()) > 0
        assert np.all(got["D"][:, 1:] > 0) and not np.any(got["D"][:, 0]) and not np.any(got["C"][:, 0])
        med, mn = timed(ctx.sf_accumulate)
        ns = 2 * a.window + 1
        res["sf"] = {"ms_per_call_median": med, "ms_per_call_min": mn, "scratch_bytes": 8 * ns * 3 * ((cfg.Np + 7) // 8 * 8) * W,
                     "links_per_call": float(cfg.Np) * (ns - 1) * W}
        res["ratio_to_fqs"] = med / fmed
    if a.resources:
        res["resources"] = json.loads(a.resources)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
