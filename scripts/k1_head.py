"""Where K1's launch time goes outside the steady state (bench.py's workload: N=256, 161 beads, 128 walkers).

  PIGS_EXTRA_FLAGS=-DPIGS_EXPERIMENT_K1_CLOCK PIGS_LIB_OUT=build/libpigs_k1clock.so python -m pathintegralgroundstate_amd.build
  PIGS_LIB=build/libpigs_k1clock.so python scripts/k1_head.py [launches]     # per-wave clock records of pipe2
  python scripts/k1_head.py                                                  # product library: host enqueue time only

With the clock build, every launch's per-wave records (pigs_k1.hip, k1_clock: s_memrealtime at entry, first-item loads
and table chunks landed, past the workgroup barrier, end) are split into the head (entry -> table ready), the steady
state, the per-CU tail (last wave of the chip minus last wave of each CU) and what lies outside every wave's life
(HIP-event duration of the launch minus first entry .. last end).  Always: host enqueue time per bench.py step (the
timed loop of bench.py without its synchronisation) against the kernel time of the same steps.
"""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

TICK_US = 0.01          # s_memrealtime: 100 MHz


def pct(a, q):
    return float(np.percentile(a, q))


def main():
    launches = int(sys.argv[1]) if len(sys.argv) > 1 else 50
    import torch
    import bench
    from pathintegralgroundstate_amd import SystemConfig, api

    dev = torch.device("cuda", 0)
    cfg = SystemConfig(dim=3, Np=256, Nb=80, density=0.365, dt=5e-3, Rm=1.2)
    W = 128
    VT, WF = api.build_tables(cfg)
    nsets = 8
    Paths, sets = bench.make_workload(cfg, W, nsets, seed=1982)
    ctx = api.PigsContext(cfg, VT, WF, n_walkers=W, device_id=0)
    ctx.upload_all(Paths)
    dsets = [tuple(torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in s) for s in sets]
    n_items = len(sets[0][0])
    d_out = [torch.empty(n_items, dtype=torch.float64, device=dev) for _ in range(nsets)]

    def step(i):
        w, ip, ib, xn, xo = dsets[i % nsets]
        ctx.delta_action_batch_dev(n_items, w.data_ptr(), ip.data_ptr(), ib.data_ptr(), xn.data_ptr(),
                                   xo.data_ptr(), d_out[i % nsets].data_ptr())

    kstream = torch.cuda.ExternalStream(ctx.stream(), device=dev)
    for i in range(40):
        step(i)
    ctx.sync()
    res = {"workload": "bench.py default: %d items x %d partners" % (n_items, cfg.Np - 1)}

    # host enqueue time per step: bench.py's timed loop without the synchronisation at its end
    steps = 400
    enq = []
    for rep in range(5):
        ev0 = torch.cuda.Event(enable_timing=True)
        ev1 = torch.cuda.Event(enable_timing=True)
        ctx.sync()
        ev0.record(kstream)
        t0 = time.perf_counter()
        for i in range(steps):
            step(i)
        t1 = time.perf_counter()
        ev1.record(kstream)
        ctx.sync()
        torch.cuda.synchronize()
        enq.append({"host_enqueue_us_per_step": 1e6 * (t1 - t0) / steps,
                    "gpu_us_per_step": 1e3 * ev0.elapsed_time(ev1) / steps})
    res["enqueue"] = enq

    L = api.load_library()
    if hasattr(L, "pigs_k1_clock_read"):
        L.pigs_k1_clock_read.argtypes = [C.POINTER(C.c_uint64), C.c_int]
        props = torch.cuda.get_device_properties(dev)
        ncu = props.multi_processor_count
        nblk = min((n_items + 15) // 16, ncu)
        nw = nblk * 16
        buf = np.zeros(nw * 5, dtype=np.uint64)
        rows = []
        for i in range(launches):
            ctx.sync()
            ev0 = torch.cuda.Event(enable_timing=True)
            ev1 = torch.cuda.Event(enable_timing=True)
            ev0.record(kstream)
            step(i)
            ev1.record(kstream)
            ctx.sync()
            torch.cuda.synchronize()
            assert L.pigs_k1_clock_read(buf.ctypes.data_as(C.POINTER(C.c_uint64)), nw) == 0
            r = buf.reshape(nw, 5).astype(np.int64)
            t0 = r[:, 0].min()
            ent, lod, rdy, end, cnt = [(r[:, k] - t0) * TICK_US if k < 4 else r[:, k] for k in range(5)]
            assert cnt.sum() == n_items, (cnt.sum(), n_items)
            cu_end = end.reshape(nblk, 16).max(axis=1)
            cu_first_end = end.reshape(nblk, 16).min(axis=1)
            cu_entry = ent.reshape(nblk, 16).min(axis=1)
            rows.append({
                "event_us": 1e3 * ev0.elapsed_time(ev1),
                "span_us": float(end.max()),                                  # first wave entry .. last wave end
                "entry_spread_us": float(ent.max()),                          # dispatch of the last wave after the first
                "cu_entry_spread_us": float(cu_entry.max()),
                "own_loads_us": float(np.mean(lod - ent)),                    # entry -> own first-item loads + table chunks landed
                "own_loads_max_us": float(np.max(lod - ent)),
                "barrier_wait_us": float(np.mean(rdy - lod)),                 # landed -> past the workgroup barrier
                "head_us": float(np.mean(rdy - ent)),                         # entry -> table ready
                "head_max_us": float(np.max(rdy - ent)),
                "ready_abs_max_us": float(rdy.max()),
                "work_us": float(np.mean(end - rdy)),
                "life_us": float(np.mean(end - ent)),
                "cu_tail_mean_us": float(np.mean(end.max() - cu_end)),        # last wave of the chip minus last wave of the CU
                "cu_tail_p90_us": pct(end.max() - cu_end, 90),
                "in_cu_tail_mean_us": float(np.mean(cu_end - cu_first_end)),  # last minus first wave end inside a CU
                "items_per_cu_min": int(cnt.reshape(nblk, 16).sum(axis=1).min()),
                "items_per_cu_max": int(cnt.reshape(nblk, 16).sum(axis=1).max()),
            })
        keys = rows[0].keys()
        res["clock"] = {"launches": launches, "cus": nblk,
                        "median": {k: float(np.median([x[k] for x in rows])) for k in keys},
                        "min": {k: float(np.min([x[k] for x in rows])) for k in keys},
                        "max": {k: float(np.max([x[k] for x in rows])) for k in keys}}
        res["clock"]["median"]["outside_waves_us"] = res["clock"]["median"]["event_us"] - res["clock"]["median"]["span_us"]
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
