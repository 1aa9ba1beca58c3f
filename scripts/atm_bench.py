"""Time pigs_atm_accumulate beside pigs_g3_accumulate (Nr = 10, Na = 20, the same radius) and pigs_vh_accumulate (Ntau = 0)
on the same context and window, at config 3's shape (Np 256, 161 beads, 128 walkers, window 20, random in-box worldlines):
the cutoff at half the box and at a first-shell radius (--shell, in the units of the box).

Every call is timed by two events on the context's stream, after one warm-up call of the same shape; the figures are
medians (and minima) over --calls calls.  The triplets of a call are counted by the device itself (the sum of `ntrip`
after one call); g3's are the sum of its `trip`, the pairs of legs of every vertex, of which the three-body sum visits one
third (each triangle from its lowest vertex only) and keeps those whose third side is within the cutoff too.  Prints one
JSON line and writes it to --out when given.

Not measured here: the cost per MC step in a front-end run, 2D, shapes other than config 3's.

  python scripts/atm_bench.py [--window 20] [--calls 5] [--shell 1.9] [--out profiles/atm_bench.json]
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
    res = {"Np": cfg.Np, "beads": cfg.path_shape[0], "walkers": W, "window": a.window, "calls": a.calls,
           "half_box": half, "g3_Nr": 10, "g3_Na": 20, "atm": []}
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

        ctx.vh_init(0, a.window, 100, cfg.rcut / 100, 100, cfg.rcut / 100)
        vmed, vmin = timed(ctx.vh_accumulate)
        res["vh_ntau0"] = {"ms_per_call_median": vmed, "ms_per_call_min": vmin}
        for rname, rc in (("shell", a.shell), ("half_box", half)):
            ctx.g3_init(10, rc / 10, 20, a.window)
            ctx.g3_accumulate()
            leg_pairs = int(ctx.g3_read(reset=True)["trip"].sum())
            gmed, gmin = timed(ctx.g3_accumulate)
            ctx.atm_init(rc, a.window)
            ctx.atm_accumulate()
            got = ctx.atm_read(reset=True)
            triplets = int(got["ntrip"].sum())
            assert got["samples"].tolist() == [1] * W
            med, mn = timed(ctx.atm_accumulate)
            res["atm"].append({"radius": rname, "rc": rc, "ms_per_call_median": med, "ms_per_call_min": mn,
                               "triplets_per_call": triplets, "triplets_per_slice": triplets / float(W * ns),
                               "triplets_per_second": triplets / (med * 1e-3),
                               "leg_pairs_visited_per_call": leg_pairs // 3,
                               "leg_pairs_visited_per_second": (leg_pairs // 3) / (med * 1e-3),
                               "g3_same_radius": {"ms_per_call_median": gmed, "ms_per_call_min": gmin,
                                                  "leg_pairs_per_call": leg_pairs},
                               "ratio_to_g3_same_radius": med / gmed, "ratio_to_vh_ntau0": med / vmed})
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
