"""Time pigs_grv_accumulate in both forms of its vector histogram (global u64 atomics, grid privatised in LDS) against the
only earlier route to a windowed g(r) in the same process -- pigs_structure_batch once per window slice, radial only,
one synchronisation per call -- at config 3's shape (Np 256, 161 beads, 128 walkers, random in-box worldlines).

Host wall clock over `--calls` queued calls closed by one read (which synchronises), after a warm-up of the same shape,
best of `--repeats` and median.  Prints one JSON line and writes it to --out when given.

  python scripts/grv_bench.py [--nbin 32] [--window 20] [--calls 10] [--repeats 5] [--only global|lds|auto|structure]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pathintegralgroundstate_amd import SystemConfig, api  # noqa: E402

FORMS = {"global": 0, "lds": 1, "auto": -1}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nbin", type=int, nargs="+", default=[32])
    ap.add_argument("--window", type=int, default=20)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--walkers", type=int, default=128)
    ap.add_argument("--only", choices=list(FORMS) + ["structure"], default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert api.device_count() >= 1, "needs a GPU"
    cfg = SystemConfig(dim=3, Np=256, Nb=80, density=0.365)
    VT, WF = api.build_tables(cfg)
    W = a.walkers
    P = np.random.default_rng(1982).uniform(-0.5, 0.5, (W,) + tuple(cfg.path_shape)) * np.asarray(cfg.Lbox[:3])
    ns = 2 * a.window + 1
    pairs = float(cfg.Np * (cfg.Np - 1) // 2) * ns * W
    res = {"Np": cfg.Np, "beads": cfg.path_shape[0], "walkers": W, "window": a.window, "calls": a.calls, "Nr": cfg.Nbin,
           "pairs_per_call": pairs, "grv": []}
    with api.PigsContext(cfg, VT, WF, n_walkers=W) as ctx:
        ctx.upload_all(P)

        def timed(acc, read):
            acc()
            read()                                          # warm-up of this shape
            t = []
            for _ in range(a.repeats):
                t0 = time.perf_counter()
                for _ in range(a.calls):
                    acc()
                read()
                t.append((time.perf_counter() - t0) / a.calls)
            return min(t), sorted(t)[len(t) // 2]

        for nbin in a.nbin:
            for name, form in FORMS.items():
                if a.only not in (None, name):
                    continue
                ctx.set_tuning("grv_form", form)
                ctx.grv_init(nbin, a.window)
                try:
                    best, med = timed(ctx.grv_accumulate, lambda: ctx.grv_read(reset=True))
                except api.PigsError as e:                  # a forced LDS form whose grid does not fit
                    res["grv"].append({"Nbin": nbin, "form": name, "refused": str(e)})
                    continue
                res["grv"].append({"Nbin": nbin, "form": name, "ms_per_call_min": best * 1e3, "ms_per_call_median": med * 1e3,
                                   "pairs_per_s": pairs / best})
        ctx.set_tuning("grv_form", -1)
        if a.only in (None, "structure"):
            def window_loop():
                for ib in range(cfg.Nb - a.window, cfg.Nb + a.window + 1):
                    ctx.structure_batch(ib, cfg.Nbin, cfg.rbin, 1)
            best, med = timed(window_loop, lambda: None)
            res["structure_batch_per_slice"] = {"calls_per_sample": ns, "ms_per_sample_min": best * 1e3,
                                                "ms_per_sample_median": med * 1e3, "pairs_per_s": pairs / best,
                                                "note": "radial only, one synchronisation per slice"}
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
