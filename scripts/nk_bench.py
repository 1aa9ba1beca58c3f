"""Time pigs_nk_accumulate beside the sampler's own MC step, at config 3's shape (Np 256, 161 beads) with the worm sector on
(CWorm 0.5, swapping, Nobdm 10: the worm configuration of scripts/sampler_bench.py and bench.py), at --walkers 128,1024
and --nmax 3,8 (nbin 32).

Every call is timed by two events on the context's stream, after --warm steps that let walkers open and one warm-up call of
the same shape; the figures are medians (and minima) over --calls calls, each accumulate following a step of its own, and
the accumulate is set against the step time measured in the same run.  The work of a call follows the number of open
walkers of that step, which is recorded.  One accumulate is a single launch of some 10 to 100 us between two events, close to
the events' resolution and to the launch overhead: its fraction of a step is an order of magnitude, not a figure to
compare kernels by.  Prints one JSON line and writes it to --out when given.

Not measured here: 2D, other shapes, the host-driven path (pigs_nk_add).

  python scripts/nk_bench.py [--walkers 128,1024] [--nmax 3,8] [--calls 7] [--out profiles/nk_bench.json]
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bench import make_workload  # noqa: E402
from pathintegralgroundstate_amd import SystemConfig, api  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--walkers", default="128,1024")
    ap.add_argument("--nmax", default="3,8")
    ap.add_argument("--nbin", type=int, default=32)
    ap.add_argument("--nobdm", type=int, default=10)
    ap.add_argument("--calls", type=int, default=7)
    ap.add_argument("--warm", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    assert api.device_count() >= 1 and torch.cuda.is_available(), "needs a GPU"
    res = {"Np": 256, "beads": 161, "CWorm": 0.5, "Nobdm": a.nobdm, "nbin": a.nbin, "calls": a.calls, "runs": []}
    for W in [int(x) for x in a.walkers.split(",")]:
        cfg = SystemConfig(dim=3, Np=256, Nb=80, Nlev=4, Nstag=5, Lstag=32, CMFreq=1, delta_cm=0.12)
        VT, WF = api.build_tables(cfg)
        Paths, _ = make_workload(cfg, W, 1, 1982)
        with api.PigsContext(cfg, VT, WF, n_walkers=W) as ctx:
            ctx.upload_all(Paths)
            ctx.sampler_init(CWorm=0.5, swapping=True, Nobdm=a.nobdm)
            xe = np.repeat(Paths[:, cfg.Nb, cfg.Np - 1][:, None, :], 2, axis=1)
            ctx.sampler_set_worm(np.zeros(W, np.int32), np.zeros(W, np.int32), xe)
            for w in range(W):
                ctx.sampler_seed(w, 1982 + w)
            ks = torch.cuda.ExternalStream(ctx.stream(), device=torch.device("cuda", torch.cuda.current_device()))
            istep = 0
            for _ in range(a.warm):
                istep += 1
                ctx.sampler_step(istep)
            ctx.sync()
            for nmax in [int(x) for x in a.nmax.split(",")]:
                ctx.nk_init(nmax, a.nbin)
                ctx.nk_accumulate()
                ctx.sync()                                  # warm-up of this shape
                ctx.nk_read(reset=True)
                step_ms, acc_ms, nopen = [], [], []
                for _ in range(a.calls):
                    e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
                    istep += 1
                    e[0].record(ks)
                    ctx.sampler_step(istep)
                    e[1].record(ks)
                    ctx.nk_accumulate()
                    e[2].record(ks)
                    e[2].synchronize()
                    step_ms.append(e[0].elapsed_time(e[1]))
                    acc_ms.append(e[1].elapsed_time(e[2]))
                    nopen.append(int(ctx.nk_read(reset=True)["nopen"].sum()) // max(a.nobdm, 1))
                sm, am = float(np.median(step_ms)), float(np.median(acc_ms))
                res["runs"].append({"walkers": W, "nmax": nmax, "vectors": int(ctx.nk_vectors().shape[0]),
                                    "step_ms_median": sm, "step_ms_min": float(min(step_ms)),
                                    "accumulate_ms_median": am, "accumulate_ms_min": float(min(acc_ms)),
                                    "accumulate_over_step": am / sm, "open_walkers_per_call": nopen})
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
