"""Time pigs_lat_accumulate beside pigs_vh_accumulate (Ntau = 0, which folds the same Np^2 separations per slice) on the
same context and window, at config 3's shape (Np = nsite 256, 161 beads, 128 walkers, window 20): the particles jittered
about the first 256 cells of a 7^3 grid in the box, +-0.15 spacings per axis and bead.

Every call is timed by two events on the context's stream, after one warm-up call of the same shape; the figures are
medians (and minima) over --calls calls.  --resources takes the kernel resource figures (a JSON object, as
scripts/kernel_regs.sh reports them for pigs_lat.hip) into the result.  Prints one JSON line and writes it to --out when
given.

Not measured here: the cost per MC step in a front-end run, 2D, shapes other than config 3's.

  python scripts/lat_bench.py [--window 20] [--calls 5] [--nbin 100] [--out profiles/lat_bench.json]
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
    ap.add_argument("--nbin", type=int, default=100)
    ap.add_argument("--resources", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    assert api.device_count() >= 1 and torch.cuda.is_available(), "needs a GPU"
    cfg = SystemConfig(dim=3, Np=a.Np, Nb=80, density=0.365)
    VT, WF = api.build_tables(cfg)
    W, L = a.walkers, np.asarray(cfg.Lbox[:3])
    n = int(np.ceil(a.Np ** (1.0 / 3.0) - 1e-9))
    idx = np.stack(np.unravel_index(np.arange(a.Np), (n,) * 3), axis=1).astype(float)
    R = (idx + 0.5) * (L / n) - 0.5 * L
    rng = np.random.default_rng(1982)
    P = R[None, None] + rng.uniform(-0.15, 0.15, (W,) + tuple(cfg.path_shape)) * (L / n)
    P = P - L * np.floor((P + 0.5 * L) / L)
    res = {"Np": cfg.Np, "nsite": len(R), "beads": cfg.path_shape[0], "walkers": W, "window": a.window, "calls": a.calls,
           "nbin": a.nbin, "rmax": 0.5 * float(L[0]) / n, "cm": 1}
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
        ctx.lat_init(R, a.nbin, res["rmax"], a.window, 1)
        ctx.lat_accumulate()
        got = ctx.lat_read(reset=True)
        assert got["samples"].tolist() == [1] * W and int(got["nlost"].sum()) == 0
        assert np.all(got["occ"][..., 1] == len(R))         # every particle at its own site
        med, mn = timed(ctx.lat_accumulate)
        res["lat"] = {"ms_per_call_median": med, "ms_per_call_min": mn,
                      "distances_per_call": float(cfg.Np) * len(R) * (2 * a.window + 1) * W,
                      "distances_per_second": float(cfg.Np) * len(R) * (2 * a.window + 1) * W / (med * 1e-3)}
        res["ratio_to_vh_ntau0"] = med / vmed
    if a.resources:
        res["resources"] = json.loads(a.resources)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
