"""Time pigs_g3_accumulate beside pigs_vh_accumulate (Ntau = 0) and pigs_grv_accumulate (Nbin = 16) on the same context
and window, at config 3's shape (Np 256, 161 beads, 128 walkers, window 20, random in-box worldlines): the radius at a
first shell (--shell, in the units of the box) and at half the box, Nr = 10 radial bins, a few Na, and both kernel forms
(g3_form 1: counters in LDS; 0: global atomics, at half the box for one Na only -- it is the fallback of grids that do not
fit the LDS, and slow there).

Every call is timed by two events on the context's stream, after one warm-up call of the same shape; the figures are
medians (and minima) over --calls calls.  The triplets of a call are counted by the device itself (the sum of `trip` after
one call).  Prints one JSON line and writes it to --out when given.

  python scripts/g3_bench.py [--window 20] [--calls 5] [--na 10 20 40] [--shell 1.9] [--out profiles/g3_bench.json]
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
    ap.add_argument("--nr", type=int, default=10)
    ap.add_argument("--na", type=int, nargs="+", default=[10, 20, 40])
    ap.add_argument("--shell", type=float, default=1.9)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    assert api.device_count() >= 1 and torch.cuda.is_available(), "needs a GPU"
    cfg = SystemConfig(dim=3, Np=a.Np, Nb=80, density=0.365)
    VT, WF = api.build_tables(cfg)
    W = a.walkers
    P = np.random.default_rng(1982).uniform(-0.5, 0.5, (W,) + tuple(cfg.path_shape)) * np.asarray(cfg.Lbox[:3])
    half = 0.5 * min(cfg.Lbox[:3])
    ns = 2 * a.window + 1
    res = {"Np": cfg.Np, "beads": cfg.path_shape[0], "walkers": W, "window": a.window, "calls": a.calls, "Nr": a.nr,
           "half_box": half, "g3": []}
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

        ctx.grv_init(16, a.window)
        gmed, gmin = timed(ctx.grv_accumulate)
        res["grv_nbin16"] = {"ms_per_call_median": gmed, "ms_per_call_min": gmin}
        ctx.vh_init(0, a.window, 100, cfg.rcut / 100, 100, cfg.rcut / 100)
        vmed, vmin = timed(ctx.vh_accumulate)
        res["vh_ntau0"] = {"ms_per_call_median": vmed, "ms_per_call_min": vmin}
        for rname, rmax in (("shell", a.shell), ("half_box", half)):
            for Na in a.na:
                for form in (1, 0):
                    if form == 0 and rname == "half_box" and Na != a.na[len(a.na) // 2]:
                        continue
                    ctx.set_tuning("g3_form", form)
                    ctx.g3_init(a.nr, rmax / a.nr, Na, a.window)
                    ctx.g3_accumulate()
                    got = ctx.g3_read(reset=True)
                    triplets, legs = int(got["trip"].sum()), int(got["pair"].sum())
                    med, mn = timed(ctx.g3_accumulate)
                    res["g3"].append({"radius": rname, "rmax": rmax, "Na": Na, "form": form, "ms_per_call_median": med,
                                      "ms_per_call_min": mn, "triplets_per_call": triplets,
                                      "legs_per_vertex": legs / float(W * ns * cfg.Np),
                                      "triplets_per_second": triplets / (med * 1e-3),
                                      "ratio_to_vh_ntau0": med / vmed, "ratio_to_grv": med / gmed})
        ctx.set_tuning("g3_form", -1)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
