"""Time pigs_cl_accumulate beside pigs_bop_accumulate (Nr = 0; the same radius and window: both do the same neighbour
pass) on one context, at config 3's shape (Np 256, 161 beads, 128 walkers, window 20): uniform random points in the cell,
the bond radius a little above the connectivity threshold of the density (0.95 rho^-1/3).

Every call is timed by two events on the context's stream, after one warm-up call of the same shape; the figures are
medians (and minima) over --calls calls.  One context, no retries.  The largest number of labelling sweeps that any
(walker, slice) of the input needed is reported beside them.  --resources takes the kernel resource figures (a JSON object,
from the gfx950 compile of pigs_cl.hip) into the result.  Prints one JSON line and writes it to --out when given.

Not measured here: the cost per MC step in a front-end run, 1D and 2D, shapes other than config 3's, the form without bit
rows (Np above 256), sampled worldlines instead of uniform points.

  timeout 300 python scripts/cl_bench.py [--window 20] [--calls 5] [--out profiles/cl_bench.json]
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
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--walkers", type=int, default=128)
    ap.add_argument("--np", type=int, default=256, dest="Np")
    ap.add_argument("--rc-factor", type=float, default=0.95)
    ap.add_argument("--resources", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    assert api.device_count() >= 1 and torch.cuda.is_available(), "needs a GPU"
    cfg = SystemConfig(dim=3, Np=a.Np, Nb=80, density=0.365)
    VT, WF = api.build_tables(cfg)
    W, L = a.walkers, np.asarray(cfg.Lbox[:3])
    rc = min(a.rc_factor * cfg.density ** (-1.0 / 3.0), 0.5 * float(L.min()))
    rng = np.random.default_rng(2026)
    P = rng.uniform(-0.5, 0.5, (W,) + tuple(cfg.path_shape)) * L
    res = {"Np": cfg.Np, "beads": cfg.path_shape[0], "walkers": W, "window": a.window, "rc": rc, "calls": a.calls}
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

        ctx.bop_init(rc, a.window, 50, 0)
        bmed, bmin = timed(ctx.bop_accumulate)
        res["bop"] = {"ms_per_call_median": bmed, "ms_per_call_min": bmin}
        ctx.cl_init(rc, a.window)
        ctx.cl_accumulate()
        got = ctx.cl_read(reset=True)
        ns = 2 * a.window + 1
        s = np.arange(1, cfg.Np + 1)
        assert got["samples"].tolist() == [ns] * W and int(got["nbond"].min()) > 0
        assert np.array_equal((s * got["nsize"]).sum(axis=1), cfg.Np * got["samples"])
        assert np.array_equal(got["nlarge"].sum(axis=1), got["samples"])
        med, mn = timed(ctx.cl_accumulate)
        tot = got["nsize"].sum(axis=0)
        res["cl"] = {"ms_per_call_median": med, "ms_per_call_min": mn, "max_sweeps": ctx.cl_sweeps(),
                     "slices_per_call": ns * W, "scratch_bytes": 8 * ns * cfg.Np * W,
                     "bonds_per_particle": float(got["nbond"].sum()) / (float(got["samples"].sum()) * cfg.Np),
                     "mean_largest_over_Np": float((s * got["nlarge"].sum(axis=0)).sum()) / (float(got["samples"].sum()) * cfg.Np),
                     "distinct_sizes": int(np.count_nonzero(tot))}
        res["ratio_to_bop"] = med / bmed
    if a.resources:
        res["resources"] = json.loads(a.resources)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
