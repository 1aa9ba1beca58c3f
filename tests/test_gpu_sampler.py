"""K6, the device-resident sampler (one launch = one MC step of every walker, no host in the
loop), against output files of the reference PROGRAM for pure diagonal PIGS runs (CWorm = 0,
sampling = 'bis'; tests/golden/vpi_runs/*_cworm0*).

What must hold: every walker draws the reference's random stream for its seed and takes the same
accept/reject decisions, so the final worldline agrees with the reference's to rounding (the
Box-Muller log() is the device library's: last-bit differences in the Gaussians, nothing else)
and the block energies agree with the 64-bit values of the reference's own estimators (driver.npz next to each
run; the program's files carry only 10 digits): V, Et, Kt to 1e-10, the mixed estimator's E, K to
helpers.MIXED_TOL (the reference's LocalEnergy itself moves by 6e-10 under one-ulp moves)."""
import os

import numpy as np
import pytest

from conftest import GOLDEN
from helpers import MIXED_TOL, block_energy_errors, driver_blocks, same_bits
from pathintegralgroundstate_amd import SystemConfig

pytestmark = pytest.mark.gpu
RUNS = os.path.join(GOLDEN, "vpi_runs")
PIGS_ERR_ARG = -1                                   # include/pigs_hip.h


def _run_device(gpu_lib, oracle, cfg, seeds, nblock, nstep):
    from oracle.pyoracle import System
    S = System(dim=cfg.dim, Np=cfg.Np, Nb=cfg.Nb, density=cfg.density, dt=cfg.dt, trap=cfg.trap,
               a_ho=cfg.a_ho, Lbox=cfg.Lbox, rcut=cfg.rcut)
    VT, WF = gpu_lib.build_tables(cfg)
    W = len(seeds)
    ctx = gpu_lib.PigsContext(cfg, VT, WF, n_walkers=W)
    ctx.sampler_init()
    Paths = []
    for w, seed in enumerate(seeds):
        P, g = oracle.init_path(S, seed)             # reference init: consumes Np*dim uniforms
        Paths.append(P)
        ctx.sampler_set_rng(w, g.mti, np.array(g.mt[:], np.uint32))
    ctx.upload_all(np.stack(Paths))
    blocks = np.zeros((W, nblock, 6))
    for ib in range(nblock):
        acc = np.zeros((W, 6))
        for istep in range(1, nstep + 1):
            ctx.sampler_step(istep)
            E1, _, _ = ctx.local_energy_batch(0)
            E2, _, _ = ctx.local_energy_batch(2 * cfg.Nb)
            Et, Kt, Pt = ctx.therm_energy_batch()
            E = 0.5 * (E1 + E2)
            acc += np.stack([E, E - Pt, Pt, Et, Kt, Pt], 1)
        blocks[:, ib] = acc / np.float32(nstep) / cfg.Np
    final = ctx.download_all()
    counters = ctx.sampler_counters()
    ctx.close()
    return blocks, final, counters


def _cfg(name):
    txt = open(os.path.join(RUNS, name, "vpi.in")).read()
    return SystemConfig.from_namelists(txt)


@pytest.mark.parametrize("names", [["he4_bis_cworm0_s1982", "he4_bis_cworm0_s1983"], ["trap2d_bis_cworm0"]])
def test_device_sampler_reproduces_reference_program(gpu_lib, oracle, names):
    cfg = _cfg(names[0])
    seeds = [_cfg(n).seed for n in names]
    blocks, final, counters = _run_device(gpu_lib, oracle, cfg, seeds, cfg.Nblock, cfg.Nstep)
    for w, n in enumerate(names):
        src = os.path.join(RUNS, n)
        want = np.load(os.path.join(src, "final_worldline.npz"))["Path"]
        L = np.asarray(cfg.Lbox[:cfg.dim])
        d = final[w] - want
        if not cfg.trap:
            d = d - L * np.round(d / L)              # a last-bit difference may sit on either side of the wrap
        assert np.max(np.abs(d)) < 1e-10, np.max(np.abs(d))
        assert same_bits(final[w], want), "device-sampler worldline is not the reference's bit for bit"
        # 64-bit block energies of the reference's own estimators (driver.npz), 1e-10 relative
        _, want_rows = driver_blocks(dict(np.load(os.path.join(src, "driver.npz"))))
        got = blocks[w]
        assert got.shape == want_rows.shape
        em, er = block_energy_errors(got, want_rows)
        assert np.all(er <= 1e-10) and np.all(em <= MIXED_TOL), (er.max(), em.max())
    assert counters.sum() > 0


def test_device_sampler_matches_host_sampler_counters(gpu_lib, oracle):
    """Same run through the host-driven Fortran sampler (bit-exact with the reference): identical
    acceptance counts, i.e. identical decisions, move by move in aggregate."""
    import subprocess
    import tempfile
    from conftest import ROOT
    host = os.path.join(ROOT, "pathintegralgroundstate_amd", "host")
    subprocess.check_call(["make", "-s", "-C", host])
    name = "he4_bis_cworm0_s1982"
    cfg = _cfg(name)
    blocks, final, counters = _run_device(gpu_lib, oracle, cfg, [cfg.seed], cfg.Nblock, cfg.Nstep)
    with tempfile.TemporaryDirectory() as td:
        with open(os.path.join(td, "vpi.in"), "w") as f:
            f.write(open(os.path.join(RUNS, name, "vpi.in")).read() + "&gpu\n device_sampler = F\n/\n")      # the host-driven sampler
        with open(os.path.join(td, "vpi.in")) as fin, open(os.path.join(td, "out.txt"), "w") as fo:
            subprocess.run([os.path.join(host, "pigs_vpi")], stdin=fin, stdout=fo, cwd=td, check=True, timeout=600)
        got = np.fromfile(os.path.join(td, "worldlines_final.bin")).reshape(final[0].shape)
    assert same_bits(final[0], got)


def _run_device_worm(gpu_lib, oracle, cfg, seeds, nblock, nstep):
    """Block loop of the reference (vpi.f90:244-545) around the device sampler with the worm sector on:
    diagonal estimators only for walkers that end the step closed; OBDM histogram from the device."""
    from oracle.pyoracle import System
    S = System(dim=cfg.dim, Np=cfg.Np, Nb=cfg.Nb, density=cfg.density, dt=cfg.dt)
    VT, WF = gpu_lib.build_tables(cfg)
    W = len(seeds)
    ctx = gpu_lib.PigsContext(cfg, VT, WF, n_walkers=W)
    ctx.sampler_init(CWorm=cfg.CWorm, swapping=cfg.swapping, Nobdm=cfg.Nobdm, Nbin=cfg.Nbin, Npw=cfg.Npw)
    Paths, xends = [], []
    for w, seed in enumerate(seeds):
        P, g = oracle.init_path(S, seed)
        Paths.append(P)
        xends.append(np.stack([P[cfg.Nb, cfg.Np - 1], P[cfg.Nb, cfg.Np - 1]]))
        ctx.sampler_set_rng(w, g.mti, np.array(g.mt[:], np.uint32))
    ctx.upload_all(np.stack(Paths))
    ctx.sampler_set_worm(np.zeros(W, np.int32), np.zeros(W, np.int32), np.stack(xends))
    rows_e = [[] for _ in range(W)]
    rows_t = [[] for _ in range(W)]
    events = [[] for _ in range(W)]
    for ib in range(nblock):
        acc = np.zeros((W, 6))
        nd = np.zeros(W, int)
        for istep in range(1, nstep + 1):
            ctx.sampler_step(istep)
            ev = ctx.sampler_events()
            for w in range(W):
                events[w] += [(int(ev[w, 2 + 2 * i]), int(ev[w, 3 + 2 * i])) for i in range(ev[w, 0])]
            closed = np.flatnonzero(ev[:, 1] == 0)
            if len(closed):
                E1, _, _ = ctx.local_energy_batch(0, closed)
                E2, _, _ = ctx.local_energy_batch(2 * cfg.Nb, closed)
                Et, Kt, Pt = ctx.therm_energy_batch(closed)
                E = 0.5 * (E1 + E2)
                acc[closed] += np.stack([E, E - Pt, Pt, Et, Kt, Pt], 1)
                nd[closed] += 1
        for w in range(W):
            if nd[w]:
                v = acc[w] / np.float32(nd[w]) / cfg.Np
                rows_e[w].append([ib + 1, *v[:3]])
                rows_t[w].append([ib + 1, *v[3:]])
    final = ctx.download_all()
    isopen, iworm, xend = ctx.sampler_get_worm()
    cnt = ctx.sampler_counters16()
    nrho = ctx.sampler_nrho()
    ctx.close()
    return rows_e, rows_t, final, events, cnt, (isopen, iworm, xend), nrho


@pytest.mark.parametrize("names", [["he4_worm_s1982", "he4_worm_s1983", "he4_worm_s1984"]])
def test_device_sampler_worm_sector_vs_reference_program(gpu_lib, oracle, names):
    """CWorm > 0: open / close / half-chain moves / swap / OBDM on the device, against the reference
    program's files for three seeds (block energies as printed, final worldline to rounding)."""
    cfg = _cfg(names[0])
    seeds = [_cfg(n).seed for n in names]
    rows_e, rows_t, final, events, cnt, worm, nrho = _run_device_worm(gpu_lib, oracle, cfg, seeds, cfg.Nblock, cfg.Nstep)
    assert cnt[:, 5].sum() > 0 and cnt[:, 7].sum() > 0, cnt[:, 4:8]      # opens and closes were accepted
    for w, n in enumerate(names):
        src = os.path.join(RUNS, n)
        want = np.load(os.path.join(src, "final_worldline.npz"))["Path"]
        L = np.asarray(cfg.Lbox[:cfg.dim])
        d = final[w] - want
        d = d - L * np.round(d / L)
        assert np.max(np.abs(d)) < 1e-10, (n, np.max(np.abs(d)))
        assert same_bits(final[w], want), n
        wb, want_rows = driver_blocks(dict(np.load(os.path.join(src, "driver.npz"))))
        got_e, got_t = np.array(rows_e[w]), np.array(rows_t[w])
        assert np.array_equal(got_e[:, 0].astype(int), wb)
        got = np.concatenate([got_e[:, 1:], got_t[:, 1:]], axis=1)
        em, er = block_energy_errors(got, want_rows)
        assert np.all(er <= 1e-10) and np.all(em <= MIXED_TOL), (er.max(), em.max())


def test_worm_bookkeeping_entry_points(gpu_lib, oracle):
    """pigs_sampler_nrho's per-walker reset, the event log layout and the worm state round trip."""
    cfg = _cfg("he4_worm_s1982")
    from oracle.pyoracle import System
    S = System(dim=cfg.dim, Np=cfg.Np, Nb=cfg.Nb, density=cfg.density, dt=cfg.dt)
    VT, WF = gpu_lib.build_tables(cfg)
    W = 4
    ctx = gpu_lib.PigsContext(cfg, VT, WF, n_walkers=W)
    ctx.sampler_init(CWorm=cfg.CWorm, swapping=True, Nobdm=cfg.Nobdm, Nbin=cfg.Nbin, Npw=1)
    Paths = []
    for w in range(W):
        P, g = oracle.init_path(S, 100 + w)
        Paths.append(P)
        ctx.sampler_set_rng(w, g.mti, np.array(g.mt[:], np.uint32))
    Paths = np.stack(Paths)
    ctx.upload_all(Paths)
    xe = np.repeat(Paths[:, cfg.Nb, cfg.Np - 1][:, None, :], 2, axis=1)
    ctx.sampler_set_worm(np.zeros(W, np.int32), np.arange(1, W + 1, dtype=np.int32), xe)
    o, iw, x = ctx.sampler_get_worm()
    assert not o.any() and np.array_equal(iw, np.arange(1, W + 1)) and same_bits(x, xe)
    n_open_steps = np.zeros(W, int)
    for istep in range(1, 61):
        ctx.sampler_step(istep)
        ev = ctx.sampler_events()
        assert np.all(ev[:, 0] >= 0) and np.all(ev[:, 0] <= 1 + cfg.Nobdm) and set(np.unique(ev[:, 1])) <= {0, 1}
        for w in range(W):
            codes = ev[w, 2:2 + 2 * ev[w, 0]:2]
            assert set(codes.tolist()) <= {1, 2, 3}
        n_open_steps += ev[:, 1]
    assert n_open_steps.sum() > 0
    h = ctx.sampler_nrho()
    # every step spent open adds Nobdm end-to-end vectors inside the cutoff at most, with weight 1 in the l=0 column
    assert np.all(h[:, :, 0].sum(1) <= n_open_steps * cfg.Nobdm + 1e-9) and h[:, :, 0].sum() > 0
    assert np.array_equal(h[:, :, 0], np.round(h[:, :, 0]))
    mask = np.array([1, 0, 1, 0], np.int32)
    h2 = ctx.sampler_nrho(reset=mask)
    assert same_bits(h, h2)
    h3 = ctx.sampler_nrho()
    assert not h3[0].any() and not h3[2].any() and same_bits(h3[1], h[1]) and same_bits(h3[3], h[3])
    c = ctx.sampler_counters16()
    assert np.all(c[:, 5] <= c[:, 4]) and np.all(c[:, 7] <= c[:, 6]) and np.all(c[:, 13] <= c[:, 12])
    assert np.all(c[:, 14] <= 60 * cfg.Np) and np.all(c[:, 15] <= 60 * cfg.Nstag * cfg.Np)
    ctx.close()


def test_sampler_forms_agree(gpu_lib, oracle):
    """The two workgroup forms of K6 for periodic systems (8 waves + table image in LDS; 4 waves on the global image) cut a
    stage's Delta S into different tasks, so sums differ in the last bits -- but every decision must be the same:
    identical generator states, counters, worm flags and OBDM l=0 column, worldlines to rounding."""
    cfg = _cfg("he4_worm_s1982")
    from oracle.pyoracle import System
    S = System(dim=cfg.dim, Np=cfg.Np, Nb=cfg.Nb, density=cfg.density, dt=cfg.dt)
    VT, WF = gpu_lib.build_tables(cfg)
    W = 5
    results = {}
    for threads in (512, 256):
        ctx = gpu_lib.PigsContext(cfg, VT, WF, n_walkers=W)
        ctx.sampler_init(CWorm=cfg.CWorm, swapping=True, Nobdm=cfg.Nobdm, Nbin=cfg.Nbin, Npw=0)
        ctx.set_tuning("sweep_threads", threads)
        Paths = []
        for w in range(W):
            P, g = oracle.init_path(S, 500 + w)
            Paths.append(P)
            ctx.sampler_set_rng(w, g.mti, np.array(g.mt[:], np.uint32))
        Paths = np.stack(Paths)
        ctx.upload_all(Paths)
        xe = np.repeat(Paths[:, cfg.Nb, cfg.Np - 1][:, None, :], 2, axis=1)
        ctx.sampler_set_worm(np.zeros(W, np.int32), np.zeros(W, np.int32), xe)
        for istep in range(1, 31):
            ctx.sampler_step(istep)
        results[threads] = (ctx.download_all(), ctx.sampler_counters16(), [ctx.sampler_get_rng(w) for w in range(W)],
                            ctx.sampler_get_worm(), ctx.sampler_nrho())
        ctx.close()
    ref, got = results[512], results[256]
    L = np.asarray(cfg.Lbox[:cfg.dim])
    d = got[0] - ref[0]
    assert np.max(np.abs(d - L * np.round(d / L))) < 1e-10
    assert np.array_equal(got[1], ref[1])
    for a, b in zip(got[2], ref[2]):
        assert a[0] == b[0] and np.array_equal(np.asarray(a[1]), np.asarray(b[1]))
    assert np.array_equal(got[3][0], ref[3][0]) and np.array_equal(got[3][1], ref[3][1])
    assert np.max(np.abs(got[3][2] - ref[3][2])) < 1e-10
    assert np.array_equal(got[4][:, :, 0], ref[4][:, :, 0])


def test_sampler_forms_agree_on_long_chains(gpu_lib, oracle):
    """The same on chains long enough for everything the 8-wave form adds (33 and 81 beads, worm sector, 120 MC steps =
    ~3 10^5 stages per walker): speculative proposals of the next bisection level, TranslateChain on several CUs per walker
    -- against the 4-wave form, which has neither, and the stage-machine kernel.  Every decision identical, worldlines to
    rounding: rare paths (a window of candidates that does not suffice, a stream refill between stages, a uniform of the
    accept-without-draw kind) would show up as a different generator state."""
    from oracle.pyoracle import System
    for Np, Nb, dens in ((48, 16, 0.3), (130, 40, 0.365)):
        cfg = SystemConfig(dim=3, Np=Np, Nb=Nb, density=dens, dt=5e-3, Rm=1.2, Nlev=4, Nstag=2, Lstag=8, CMFreq=1,
                           delta_cm=0.3, CWorm=0.5, Nobdm=3, Nbin=50, Npw=0)
        S = System(dim=3, Np=Np, Nb=Nb, density=dens, dt=5e-3, Rm=1.2)
        VT, WF = gpu_lib.build_tables(cfg)
        W = 3
        results = {}
        for form in ("8 waves", "4 waves", "stage machine", "8 waves, TranslateChain in the sweep kernel"):
            ctx = gpu_lib.PigsContext(cfg, VT, WF, n_walkers=W)
            ctx.sampler_init(CWorm=cfg.CWorm, swapping=True, Nobdm=cfg.Nobdm, Nbin=cfg.Nbin, Npw=0)
            if form == "4 waves":
                ctx.set_tuning("sweep_threads", 256)
            if form == "stage machine":
                ctx.set_tuning("sweep_split", 1)
            if form.endswith("sweep kernel"):
                ctx.set_tuning("cm_split", 0)
            Paths = []
            for w in range(W):
                P, g = oracle.init_path(S, 900 + w)
                Paths.append(P)
                ctx.sampler_set_rng(w, g.mti, np.array(g.mt[:], np.uint32))
            Paths = np.stack(Paths)
            ctx.upload_all(Paths)
            xe = np.repeat(Paths[:, cfg.Nb, cfg.Np - 1][:, None, :], 2, axis=1)
            ctx.sampler_set_worm(np.zeros(W, np.int32), np.zeros(W, np.int32), xe)
            for istep in range(1, 121):
                ctx.sampler_step(istep)
            results[form] = (ctx.download_all(), ctx.sampler_counters16(), [ctx.sampler_get_rng(w) for w in range(W)],
                             ctx.sampler_get_worm(), ctx.sampler_nrho())
            ctx.close()
        ref = results["8 waves"]
        assert ref[1][:, 0].min() > 0 and ref[1][:, 3].min() > 0           # TranslateChain and Bisection moves were accepted
        L = np.asarray(cfg.Lbox[:cfg.dim])
        for form, got in results.items():
            d = got[0] - ref[0]
            assert np.max(np.abs(d - L * np.round(d / L))) < 1e-9, form
            assert np.array_equal(got[1], ref[1]), form
            for a, b in zip(got[2], ref[2]):
                assert a[0] == b[0] and np.array_equal(np.asarray(a[1]), np.asarray(b[1])), form
            assert np.array_equal(got[3][0], ref[3][0]) and np.array_equal(got[3][1], ref[3][1]), form
            assert np.array_equal(got[4][:, :, 0], ref[4][:, :, 0]), form


def _untemper(y):
    """Inverse of MT19937's tempering: the raw state word whose output is y."""
    y ^= y >> 18
    y ^= (y << 15) & 0xefc60000
    t = y
    for _ in range(5):
        t = y ^ ((t << 7) & 0x9d2c5680)
    y = t & 0xffffffff
    t = y
    for _ in range(3):
        t = y ^ (t >> 11)
    return t & 0xffffffff


@pytest.mark.parametrize("sampling", ["bis", "sta"])
def test_uniform_of_exactly_one_stays_inside_the_chain(gpu_lib, oracle, sampling):
    """Quirk Q15: grnd() divides by 2^32-1, so a uniform can be exactly 1.0 and `int((2Nb-2^Nlev+1)*u)` then points
    one bead past the chain (the reference runs off its array there).  K6 clamps the start bead: poison one state
    word of walker 0 at a time with the word that tempers to 0xFFFFFFFF -- wherever it lands (segment choice, worm
    index, Gaussian pair, Metropolis uniform) walker 1, whose beads follow walker 0's in memory, must come out
    bit-identical to the unpoisoned run, and walker 0 must stay finite and inside the box."""
    from oracle.pyoracle import System
    cfg = SystemConfig(dim=3, Np=5, Nb=8, density=0.3, dt=2e-2, Lstag=8, Nlev=3, Nstag=2, CMFreq=2,
                       CWorm=0.5, Nobdm=2, swapping=True, sampling=sampling, Nmax=2000)
    S = System(dim=3, Np=5, Nb=8, density=0.3, dt=2e-2, Nmax=2000)
    VT, WF = gpu_lib.build_tables(cfg)
    poison = _untemper(0xffffffff)
    P0, g0 = oracle.init_path(S, 11)
    P1, g1 = oracle.init_path(S, 12)
    mt0 = np.array(g0.mt[:], np.uint32)
    assert g0.mti < 600
    ctx = gpu_lib.PigsContext(cfg, VT, WF, n_walkers=2)
    ctx.sampler_init(CWorm=cfg.CWorm, swapping=True, Nobdm=cfg.Nobdm, Nbin=cfg.Nbin, Npw=0, sampling=sampling)

    def run(words):
        ctx.upload_all(np.stack([P0, P1]))
        ctx.sampler_set_rng(0, g0.mti, words)
        ctx.sampler_set_rng(1, g1.mti, np.array(g1.mt[:], np.uint32))
        xe = np.stack([np.stack([P[cfg.Nb, cfg.Np - 1]] * 2) for P in (P0, P1)])
        ctx.sampler_set_worm(np.array([1, 0], np.int32), np.array([2, 0], np.int32), xe)   # walker 0 starts open
        ctx.sampler_step(1)
        return ctx.download_all()

    base = run(mt0)
    hit = 0
    L = np.asarray(cfg.Lbox)
    for k in range(g0.mti, g0.mti + 160):
        w = mt0.copy()
        w[k] = poison
        got = run(w)
        assert same_bits(got[1], base[1]), k
        assert np.all(np.isfinite(got[0])) and np.all(np.abs(got[0]) <= L / 2 + 1e-12), k
        hit += not same_bits(got[0], base[0])
    assert hit > 40                                   # the poisoned word was consumed in most runs
    ctx.close()


def test_translate_chain_exchange_time_out_is_an_error_not_a_result(gpu_lib, oracle):
    """pigs_cm.hip runs a walker's TranslateChain on H cooperating workgroups that wait for each other's Delta S in a
    plain (non-cooperative) launch.  The waiting is bounded; this forces the bound once (test-only tuning key
    "cm_fault": every walker's last range withholds its values, the waiting workgroups give up after 2048 polls) and
    asserts what the library promises then: the launch ends (bounded run time), nothing is committed after the time-out,
    the next synchronisation returns PIGS_ERR_HIP, pigs_sampler_step refuses to go on, and no entry point hands out the
    context's state (worldlines, counters, estimators) as if it were valid."""
    import time
    from oracle.pyoracle import System
    cfg = SystemConfig(dim=3, Np=48, Nb=16, density=0.3, dt=5e-3, Rm=1.2, Nlev=4, Nstag=1, Lstag=8, CMFreq=1, delta_cm=0.3)
    S = System(dim=3, Np=48, Nb=16, density=0.3, dt=5e-3, Rm=1.2)
    VT, WF = gpu_lib.build_tables(cfg)
    W = 3
    ctx = gpu_lib.PigsContext(cfg, VT, WF, n_walkers=W)
    try:
        ctx.sampler_init()
        ctx.set_tuning("cm_split", 2)
        Paths = []
        for w in range(W):
            P, g = oracle.init_path(S, 700 + w)
            Paths.append(P)
            ctx.sampler_set_rng(w, g.mti, np.array(g.mt[:], np.uint32))
        ctx.upload_all(np.stack(Paths))
        ctx.sampler_step(1)                       # healthy step first: the exchange works
        ctx.sync()
        before = ctx.download_all()
        ctx.set_tuning("cm_fault", 1)
        t0 = time.perf_counter()
        ctx.sampler_step(2)                       # the launch itself is asynchronous and succeeds
        with pytest.raises(gpu_lib.PigsError, match="timed out"):
            ctx.sync()
        assert time.perf_counter() - t0 < 5.0     # bounded: one give-up per workgroup, then nobody waits
        for call in (lambda: ctx.sampler_step(3), ctx.download_all, ctx.sampler_counters16, ctx.therm_energy_batch,
                     lambda: ctx.sampler_get_rng(0), lambda: ctx.diagonal_estimators(structure=False)):
            with pytest.raises(gpu_lib.PigsError, match="timed out"):
                call()
        ctx.set_tuning("cm_fault", 0)             # the context stays invalid: it has to be recreated
        with pytest.raises(gpu_lib.PigsError, match="timed out"):
            ctx.sampler_step(3)
    finally:
        ctx.close()
    assert before.shape == (W, cfg.M, cfg.Np, 3)


def test_diagonal_estimators_one_call_equals_the_separate_calls(gpu_lib, oracle):
    """pigs_diagonal_estimators (one synchronisation per MC step) returns exactly what LocalEnergy x2, ThermEnergy and the
    structure call return one by one -- same kernels, same bits -- for all walkers and for a subset."""
    from oracle.pyoracle import System
    cfg = SystemConfig(dim=3, Np=64, Nb=12, density=0.3, dt=5e-3, Rm=1.2)
    S = System(dim=3, Np=64, Nb=12, density=0.3, dt=5e-3, Rm=1.2)
    VT, WF = gpu_lib.build_tables(cfg)
    rng = np.random.default_rng(5)
    W = 5
    Paths = []
    for w in range(W):
        P, _ = oracle.init_path(S, 40 + w)
        P = P + rng.normal(0, 0.15, P.shape)
        L = S.Lbox[0]
        P = np.where(P > L / 2, P - L, P)
        Paths.append(np.where(P < -L / 2, P + L, P))
    with gpu_lib.PigsContext(cfg, VT, WF, n_walkers=W) as ctx:
        ctx.upload_all(np.stack(Paths))
        for walkers in (None, np.array([3, 1], np.int32)):
            one = ctx.diagonal_estimators(40, cfg.rcut / 40, 7, walkers=walkers)
            a = ctx.local_energy_batch(0, walkers)
            b = ctx.local_energy_batch(2 * cfg.Nb, walkers)
            t = ctx.therm_energy_batch(walkers)
            gr, Sk = ctx.structure_batch(cfg.Nb, 40, cfg.rcut / 40, 7, walkers)
            for k, v in zip(("E1", "K1", "V1", "E2", "K2", "V2", "Et", "Kt", "Vt"), list(a) + list(b) + list(t)):
                assert same_bits(one[k], v), k
            assert same_bits(one["gr"], gr) and same_bits(one["Sk"], Sk)


def test_overlapped_estimators_see_the_snapshot_not_the_next_step(gpu_lib, oracle):
    """pigs_diagonal_estimators_begin / _end: the estimators of step n run on the context's second stream on a SNAPSHOT of
    the worldlines while step n+1 is sampled on the first.  Their results must be those of the synchronous call made
    between the two steps, bit for bit (same kernels, bit-identical copy), for several steps in a row and for a subset of
    the walkers; a second _begin without _end and an _end without _begin are refused, and an _end with a null output
    is refused without dropping the pending batch."""
    from oracle.pyoracle import System
    cfg = SystemConfig(dim=3, Np=48, Nb=16, density=0.3, dt=5e-3, Rm=1.2, Nlev=4, Nstag=2, Lstag=8, CMFreq=1, delta_cm=0.3)
    S = System(dim=3, Np=48, Nb=16, density=0.3, dt=5e-3, Rm=1.2)
    VT, WF = gpu_lib.build_tables(cfg)
    W = 4

    def fresh():
        ctx = gpu_lib.PigsContext(cfg, VT, WF, n_walkers=W)
        ctx.sampler_init()
        Paths = []
        for w in range(W):
            P, g = oracle.init_path(S, 300 + w)
            Paths.append(P)
            ctx.sampler_set_rng(w, g.mti, np.array(g.mt[:], np.uint32))
        ctx.upload_all(np.stack(Paths))
        return ctx
    keys = ("E1", "K1", "V1", "E2", "K2", "V2", "Et", "Kt", "Vt", "gr", "Sk")
    # reference: step, synchronous estimators, step, ...
    a = fresh()
    want = []
    for istep in range(1, 6):
        a.sampler_step(istep)
        want.append(a.diagonal_estimators(30, cfg.rcut / 30, 5))
    wa = a.download_all()
    a.close()
    # overlapped: step n+1 is queued BEFORE the estimators of step n are collected
    b = fresh()
    got = []
    b.sampler_step(1)
    for istep in range(2, 7):
        b.diagonal_estimators_begin(30, cfg.rcut / 30, 5)
        with pytest.raises(gpu_lib.PigsError, match="pending"):
            b.diagonal_estimators_begin(30, cfg.rcut / 30, 5)
        if istep <= 5:
            b.sampler_step(istep)
        # a null output is refused before anything changes: the batch stays pending and is collected below
        assert b.L.pigs_diagonal_estimators_end(b.h, None, None, None) == PIGS_ERR_ARG
        assert b"null output" in b.L.pigs_last_error()
        got.append(b.diagonal_estimators_end())
    with pytest.raises(gpu_lib.PigsError, match="pending"):
        b.diagonal_estimators_end()
    assert same_bits(b.download_all(), wa)
    for n, (g, w_) in enumerate(zip(got, want)):
        for k in keys:
            assert same_bits(g[k], w_[k]), (n, k)
    # a subset, without the structural estimators
    sub = np.array([2, 0], np.int32)
    ref = b.diagonal_estimators(walkers=sub, structure=False)
    b.diagonal_estimators_begin(walkers=sub, structure=False)
    r = b.diagonal_estimators_end()
    for k in keys[:9]:
        assert same_bits(r[k], ref[k]), k
    assert r["gr"] is None
    b.close()


def test_contexts_with_overlapped_estimators_leave_no_device_memory_behind(gpu_lib):
    """pigs_ctx_destroy releases everything a context allocated, the buffers of the overlapped estimators included (they
    leaked ~0.8 MB per context at 128 walkers x 161 beads).  22 contexts in a row, each with one _begin / _end batch: the
    free device memory after the 22nd is that after the 2nd, to within half of what 20 leaked sets would take."""
    import ctypes as C
    import gc
    cfg = SystemConfig(dim=3, Np=256, Nb=80)
    VT, WF = gpu_lib.build_tables(cfg)
    W = 128
    L = cfg.Lbox[0]
    Paths = np.random.default_rng(5).uniform(-L / 2, L / 2, (W,) + cfg.path_shape)
    hip = gpu_lib.load_library()                     # hipMemGetInfo of the HIP runtime libpigs_hip runs on
    hip.hipMemGetInfo.argtypes = [C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]

    def free_bytes():
        f, t = C.c_size_t(), C.c_size_t()
        assert hip.hipMemGetInfo(C.byref(f), C.byref(t)) == 0
        return f.value
    gc.collect()                                     # contexts earlier tests left to the garbage collector
    free = {}
    for cycle in range(1, 23):
        ctx = gpu_lib.PigsContext(cfg, VT, WF, n_walkers=W)
        ctx.upload_all(Paths)
        ctx.diagonal_estimators_begin(structure=False)
        ctx.diagonal_estimators_end()
        ctx.close()
        if cycle in (2, 22):
            free[cycle] = free_bytes()

    def reserved(n, itemsize):                       # the grow-only scratch: a quarter and 64 elements of slack
        return (n + n // 4 + 64) * itemsize
    nslot = W * 2 * cfg.Nb
    leaked_set = reserved(nslot + W, 4) + reserved(nslot, 4) + reserved(3 * nslot, 8) + reserved(9 * W, 8)
    assert free[2] - free[22] < 10 * leaked_set, (free[2] - free[22], leaked_set)


def test_translate_chain_kernel_steps_aside_when_the_chain_does_not_fit_one_workgroup(gpu_lib, oracle):
    """pigs_cm.hip holds a workgroup's bead range in LDS with a thread per coordinate: 321 beads fit two workgroups per
    walker but not one (966 rows, 165 KB).  When H is lowered to 1 -- cm_split = 1, or a second live context on the device
    (the sharded front end on one GPU, bench.py's extra legs) -- TranslateChain must stay inside the sweep kernel instead of
    failing the step with 'invalid argument' (round 3).  Same trajectory as cm_split = 0 and as two workgroups per walker."""
    from oracle.pyoracle import System
    cfg = SystemConfig(dim=3, Np=12, Nb=160, density=0.3, dt=5e-3, Rm=1.2, Nlev=4, Nstag=1, Lstag=8, CMFreq=1, delta_cm=0.3)
    S = System(dim=3, Np=12, Nb=160, density=0.3, dt=5e-3, Rm=1.2)
    VT, WF = gpu_lib.build_tables(cfg)
    res = {}
    for cm in (0, 1, 2):
        ctx = gpu_lib.PigsContext(cfg, VT, WF, n_walkers=2)
        ctx.sampler_init()
        ctx.set_tuning("cm_split", cm)
        Paths = []
        for w in range(2):
            P, g = oracle.init_path(S, 60 + w)
            Paths.append(P)
            ctx.sampler_set_rng(w, g.mti, np.array(g.mt[:], np.uint32))
        ctx.upload_all(np.stack(Paths))
        for istep in range(1, 4):
            ctx.sampler_step(istep)
        res[cm] = (ctx.download_all(), ctx.sampler_counters16())
        ctx.close()
    assert res[0][1][:, 14].min() > 0
    for cm in (1, 2):
        assert same_bits(res[cm][0], res[0][0]) and np.array_equal(res[cm][1], res[0][1]), cm


def test_two_sampling_contexts_on_one_device_share_it_through_the_translate_chain_gate(gpu_lib, oracle):
    """Two walker shards sampling on ONE GPU at once (tuning key "cm_shared"; the front end's `n_gpus = 2, same_device = T`):
    their TranslateChain kernels -- cooperating workgroups that must all be resident -- are chained through one event per
    device, each on H = 3 CUs per walker next to the other shard's sweep kernel, steps queued alternately without a
    synchronisation in between.  Every walker's trajectory is the one a single context of all walkers gives (bit for bit);
    scripts/k6_stagger.py times the staggered schedule this produces at the BASELINE size (38.5 against 39.9 ms per MC step)."""
    from oracle.pyoracle import System
    kw = dict(dim=3, Np=24, Nb=20, density=0.3, dt=5e-3, Rm=1.2)
    cfg = SystemConfig(Nlev=3, Nstag=2, Lstag=8, CMFreq=1, delta_cm=0.3, **kw)
    S = System(**kw)
    VT, WF = gpu_lib.build_tables(cfg)
    W, nstep = 12, 6
    start = [oracle.init_path(S, 300 + w) for w in range(W)]

    def run(groups, shared):
        ctxs = []
        for lo, hi in groups:
            c = gpu_lib.PigsContext(cfg, VT, WF, n_walkers=hi - lo)
            c.sampler_init()
            if shared:
                c.set_tuning("cm_shared", 1)
                c.set_tuning("cm_split", 3)
            for w in range(lo, hi):
                c.sampler_set_rng(w - lo, start[w][1].mti, np.array(start[w][1].mt[:], np.uint32))
            c.upload_all(np.stack([start[w][0] for w in range(lo, hi)]))
            ctxs.append(c)
        for istep in range(1, nstep + 1):
            for c in ctxs:
                c.sampler_step(istep)
        out = np.concatenate([c.download_all() for c in ctxs])
        cnt = np.concatenate([c.sampler_counters16() for c in ctxs])
        for c in ctxs:
            c.close()
        return out, cnt

    one = run([(0, W)], False)
    two = run([(0, W // 2), (W // 2, W)], True)
    assert one[1][:, 14].min() > 0                                   # TranslateChain moves were tried
    assert same_bits(one[0], two[0]) and np.array_equal(one[1], two[1])
