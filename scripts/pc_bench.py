"""Time pigs_pc_accumulate beside pigs_cl_accumulate (the same radius and window: both label the same slices) on one
context, on scripts/cl_bench.py's input: config 3's shape (Np 256, 161 beads, 128 walkers, window 20), uniform random
points in the cell, the bond radius a little above the connectivity threshold of the density (0.95 rho^-1/3).

Every call is timed by two events on the context's stream, after one warm-up call of the same shape; the figures are
medians (and minima) over --calls calls.  One context, no retries.  The largest numbers of labelling and of image-number
sweeps that any (walker, slice) of the input needed are reported beside them, and so are the wrapping statistics of the
input.  No ratio is fixed in advance.  --resources takes the kernel resource figures (a JSON object, from the gfx950
compile of pigs_pc.hip) into the result.  Prints one JSON line and writes it to --out when given.

Not measured here: the cost per MC step in a front-end run, 1D and 2D, shapes other than config 3's, the form without bit
rows (Np above 256), sampled worldlines instead of uniform points, chains (the deepest image propagation).

  timeout 300 python scripts/pc_bench.py [--window 20] [--ntau 20] [--calls 5] [--out profiles/pc_bench.json]
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
    res = {"Np": cfg.Np, "beads": cfg.path_shape[0], "walkers": W, "window": a.window, "ntau": a.ntau, "rc": rc, "calls": a.calls}
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

        ctx.cl_init(rc, a.window)
        cmed, cmin = timed(ctx.cl_accumulate)
        res["cl"] = {"ms_per_call_median": cmed, "ms_per_call_min": cmin, "max_sweeps": ctx.cl_sweeps()}
        ns = 2 * a.window + 1

        def pc(ntau):
            ctx.pc_init(rc, a.window, ntau)
            ctx.pc_accumulate()
            got = ctx.pc_read(reset=True)
            assert got["samples"].tolist() == [ns] * W
            assert np.array_equal(got["mwrap"].sum(axis=1), cfg.Np * got["samples"])
            assert np.array_equal(got["first"][:, 0], got["both"][:, 0])
            med, mn = timed(ctx.pc_accumulate)
            label_sweeps, image_sweeps = ctx.pc_sweeps()
            S = float(got["samples"].sum())
            return got, {"ms_per_call_median": med, "ms_per_call_min": mn, "label_sweeps": label_sweeps,
                         "image_sweeps": image_sweeps, "slices_per_call": ns * W, "scratch_bytes": 12 * ns * cfg.Np * W,
                         "wrapping_slices": float(got["swrap"][:, 1:].sum()) / S,
                         "slices_wrapping_all_axes": float(got["swrap"][:, 7].sum()) / S,
                         "p_inf": float(got["mwrap"][:, 1:].sum()) / (S * cfg.Np)}

        got, res["pc"] = pc(a.ntau)
        with np.errstate(all="ignore"):
            res["pc"]["persistence_last_lag"] = float(got["both"][:, -1].sum() / got["first"][:, -1].sum())
        _, res["pc_ntau0"] = pc(0)                          # the labelling, image numbers and wrap check alone
        res["ratio_to_cl"] = res["pc"]["ms_per_call_median"] / cmed
        res["ratio_to_cl_ntau0"] = res["pc_ntau0"]["ms_per_call_median"] / cmed
    if a.resources:
        res["resources"] = json.loads(a.resources)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
