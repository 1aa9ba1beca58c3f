"""K6, the device-resident sampler, at the BASELINE sizes -- config 3 (liquid 4He N=256, 161 beads, stock schedule)
and config 5 (N=256, 321 beads, worm sector with swaps and partial-wave OBDM; Aziz table as the reference program
runs it, and the dipolar r^-3 table fed in at the table boundary) -- against the reference's own movers and
estimators run in the program's schedule (tests/golden/vpi_runs/c3_* / c5_*: driver.npz written by
tests/golden/ref_driver.py, which is itself checked bit for bit against the reference PROGRAM).

At N=256 the kernels run what no N<=64 fixture reaches: four 64-partner passes per bead, the four-wave split of the lone
end bead, the table image in LDS next to 321-bead proposal buffers; both forms of the diagonal bisection moves are run
(inside the one-launch kernel, and the stage machine of pigs_diag.hip).

What must hold, walker by walker: the generator ends in the reference's state word for word (every random number was
consumed at the same place), the 16 attempt / accept counters and the event log (open / close / swap accepted, in
order) are identical, the worm state is the reference's, the final worldline is BIT-identical (SHA-256 of every coordinate:
the sampler's Box-Muller log() is the host libm's to the bit, csrc/pigs_log_host.h), every diagonal step's E, K, V, Et, Kt
agree to 1e-10 (64-bit reference values, no printing floor; V against |V|, the sums of opposite-sign terms against
|K|+|V| resp. |Kt|+|V|) and the OBDM histogram's l=0 column is identical."""
import os

import numpy as np
import pytest

from conftest import GOLDEN
from helpers import MIXED_TOL, check_worldline_vs_driver, fold_maxnorm, rng_sha256, run_config

pytestmark = pytest.mark.gpu
RUNS = os.path.join(GOLDEN, "vpi_runs")


def _cfg(name):
    return run_config(os.path.join(RUNS, name))


def run_k6(gpu_lib, oracle, names, threads=None, split=0, cm=None, rows=None, overlap=False):
    """The reference's block loop (vpi.f90:244-545) around pigs_sampler_step for the runs `names` (same input, one
    walker per seed).  Returns per walker: per-step rows [diag, E, Kin, Pot, Et, Kt], final worldline, counters16,
    generator state, worm state, events, OBDM histogram; and the form the sampler ran in (pigs_sampler_form).
    rows: per-walker reference answers (helpers.walker_row of a walkers.npz) in place of the runs' driver.npz -- walker w
    then runs the input of names[0] with seed rows[w]["seed"].  overlap: the diagonal steps' estimators through
    diagonal_estimators_begin / _end, queued behind the next step as the front end queues them (host/pigs_vpi.f90:
    queue_estimators, step_device), g(r) and S(k) included and summed over walkers and steps (CWorm = 0 inputs)."""
    from oracle.pyoracle import System
    cfg = _cfg(names[0])
    if rows is None:
        drv = [dict(np.load(os.path.join(RUNS, n, "driver.npz"))) for n in names]
        seeds = [_cfg(n).seed for n in names]
    else:
        drv, seeds = rows, [int(r["seed"]) for r in rows]
    assert not overlap or cfg.CWorm == 0
    pot = str(drv[0]["potential"])
    S = System(dim=cfg.dim, Np=cfg.Np, Nb=cfg.Nb, density=cfg.density, dt=cfg.dt, trap=cfg.trap, a_ho=cfg.a_ho,
               Lbox=cfg.Lbox, rcut=cfg.rcut)
    VT, WF = gpu_lib.build_tables(cfg, pot)
    W = len(drv)
    with gpu_lib.PigsContext(cfg, VT, WF, n_walkers=W) as ctx:
        ctx.sampler_init(CWorm=cfg.CWorm, swapping=cfg.swapping, Nobdm=cfg.Nobdm, Nbin=cfg.Nbin, Npw=cfg.Npw,
                         sampling=cfg.sampling)
        if threads:
            ctx.set_tuning("sweep_threads", threads)
        ctx.set_tuning("sweep_split", split)          # 1: the diagonal bisection moves in pigs_diag.hip's stage machine
        if cm is not None:
            ctx.set_tuning("cm_split", cm)            # TranslateChain by `cm` workgroups per walker (pigs_cm.hip); 0: inside the sweep kernel
        xends = []
        for w, seed in enumerate(seeds):              # one walker at a time: 1 024 worldlines of 161 beads are 1 GB
            P, g = oracle.init_path(S, seed)
            ctx.upload(w, P)
            xends.append(np.stack([P[cfg.Nb, cfg.Np - 1], P[cfg.Nb, cfg.Np - 1]]))
            ctx.sampler_set_rng(w, g.mti, np.array(g.mt[:], np.uint32))
        ctx.sampler_set_worm(np.zeros(W, np.int32), np.zeros(W, np.int32), np.stack(xends))
        steps = [[] for _ in range(W)]
        events = [[] for _ in range(W)]
        gr_sum, sk_sum = np.zeros(cfg.Nbin), np.zeros((cfg.Nk, cfg.dim))

        def collect():                                # the pending batch of diagonal_estimators_begin
            nonlocal gr_sum, sk_sum
            e = ctx.diagonal_estimators_end()
            E = 0.5 * (e["E1"] + e["E2"])
            rows_ = np.stack([np.ones(W), E, E - e["Vt"], e["Vt"], e["Et"], e["Kt"]], 1)
            gr_sum = gr_sum + e["gr"].sum(0)
            sk_sum = sk_sum + e["Sk"].sum(0)
            for w in range(W):
                steps[w].append(rows_[w])
        g = 0
        for ib in range(cfg.Nblock):
            for istep in range(1, cfg.Nstep + 1):
                g += 1
                ctx.sampler_step(istep)
                if overlap:
                    if istep > 1:                     # the previous step's estimators, computed while this step ran
                        collect()
                    ctx.diagonal_estimators_begin(cfg.Nbin, cfg.rbin, cfg.Nk)
                    continue
                if cfg.CWorm > 0:
                    ev = ctx.sampler_events()
                    isopen = ev[:, 1] != 0
                    for w in range(W):
                        events[w] += [(g, int(ev[w, 2 + 2 * i]), int(ev[w, 3 + 2 * i])) for i in range(ev[w, 0])]
                else:
                    isopen = np.zeros(W, bool)
                closed = np.flatnonzero(~isopen)
                rows_ = np.full((W, 6), np.nan)
                rows_[:, 0] = ~isopen
                if len(closed):
                    E1, _, _ = ctx.local_energy_batch(0, closed)
                    E2, _, _ = ctx.local_energy_batch(2 * cfg.Nb, closed)
                    Et, Kt, Pt = ctx.therm_energy_batch(closed)
                    E = 0.5 * (E1 + E2)
                    rows_[closed, 1:] = np.stack([E, E - Pt, Pt, Et, Kt], 1)
                for w in range(W):
                    steps[w].append(rows_[w])
            if overlap:                               # the block's last step: collected before the block ends
                collect()
        out = dict(cfg=cfg, drv=drv, steps=[np.array(s) for s in steps], final=ctx.download_all(),
                   counters=ctx.sampler_counters16(), rng=[ctx.sampler_get_rng(w) for w in range(W)],
                   worm=ctx.sampler_get_worm() if cfg.CWorm > 0 else None, events=events,
                   nrho=ctx.sampler_nrho() if cfg.CWorm > 0 and cfg.Nobdm > 0 else None, form=ctx.sampler_form(),
                   gr_sum=gr_sum if overlap else None, sk_sum=sk_sum if overlap else None)
    return out


def check_against_driver(r, w):
    cfg, drv = r["cfg"], r["drv"][w]
    # random stream: same block, same index, same words
    pos, words = r["rng"][w]
    assert int(pos) == int(drv["mti"]), (pos, drv["mti"])
    if "mt" in drv:
        assert np.array_equal(np.asarray(words, np.uint32), drv["mt"].astype(np.uint32))
    else:                                                   # a walkers.npz row keeps the words' SHA-256
        assert np.array_equal(rng_sha256(words), drv["mt_sha256"])
    # decisions
    assert np.array_equal(np.asarray(r["counters"][w], np.int64), drv["counters"]), (r["counters"][w], drv["counters"])
    assert [tuple(e) for e in r["events"][w]] == [tuple(int(x) for x in e) for e in drv["events"]]
    # worldline (L-folded max-norm on the stored beads + every bead's coordinate sums)
    worst = check_worldline_vs_driver(r["final"][w], drv, cfg.Lbox, cfg.trap, tol=0.0)      # SHA-256 of every coordinate
    # per-step energies of the diagonal steps, 64-bit reference values
    got, want = r["steps"][w], drv["steps"]
    assert got.shape == want.shape and np.array_equal(got[:, 0], want[:, 0])
    d = want[:, 0] == 1
    # E = Kin + Pot and Et = Kt + Pot are sums of terms of opposite sign (a step's E can come out near zero): the
    # scale of a row's rounding error is |Kin| + |Pot| resp. |Kt| + |Pot|, not the sum itself
    sc_e = np.abs(want[d, 2]) + np.abs(want[d, 3])
    sc_t = np.abs(want[d, 5]) + np.abs(want[d, 3])
    scale = np.stack([sc_e, sc_e, np.abs(want[d, 3]), sc_t, sc_t], 1)       # the potential energy against itself
    rel = np.abs(got[d, 1:] - want[d, 1:]) / scale
    assert np.all(rel[:, 2:] <= 1e-10), rel[:, 2:].max()                   # V, Et, Kt
    assert np.all(rel[:, :2] <= MIXED_TOL), rel[:, :2].max()   # mixed estimator: see helpers
    if r["worm"] is not None:
        isopen, iworm, xend = r["worm"]
        assert int(isopen[w]) == int(drv["isopen"])
        if int(drv["isopen"]):
            assert int(iworm[w]) == int(drv["iworm"])
        assert np.array_equal(np.asarray(xend[w]), drv["xend"])
    if r["nrho"] is not None:
        h = r["nrho"][w]                                   # (Nbin, Npw+1), accumulated over the whole run
        assert np.array_equal(h[:, 0], drv["nrho_total"][:, 0])
        assert np.all(np.abs(h - drv["nrho_total"]) <= 1e-9)
    return worst, rel.max() if d.any() else 0.0


@pytest.mark.parametrize("threads,split,cm", [(None, 0, None), (256, 0, 0), (None, 1, None), (None, 0, 0), (None, 1, 0)])
def test_k6_config3_n256_161_beads(gpu_lib, oracle, threads, split, cm):
    """Two walkers = the reference chains of seeds 1982 and 1983; default form (8 waves, table image in LDS), the
    4-wave form used beyond one walker per CU, and the stage-machine kernel (pigs_diag.hip); TranslateChain by
    cooperating workgroups (default while the chip has CUs to spare: four per walker here) and inside the sweep kernels."""
    r = run_k6(gpu_lib, oracle, ["c3_n256_s1982", "c3_n256_s1983"], threads, split, cm)
    for w in range(2):
        worst, rel = check_against_driver(r, w)
        print(f"walker {w}: worldline max |d| = {worst:.2e}, step energies max rel = {rel:.2e}")


def test_translate_chain_workgroups_do_not_change_the_trajectory(gpu_lib, oracle):
    """pigs_cm.hip cuts a walker's beads into H ranges, one workgroup each; the M values of Delta S are exchanged and
    added in bead order by every workgroup, as the one-workgroup kernel adds them: whatever H, the same bits."""
    names = ["c3_n256_s1982", "c3_n256_s1983"]
    ref = run_k6(gpu_lib, oracle, names, cm=0)
    assert ref["counters"][:, 14].min() > 0                 # TranslateChain was attempted
    for H in (1, 2, 3, 4):
        r = run_k6(gpu_lib, oracle, names, cm=H)
        assert np.array_equal(r["final"], ref["final"]), H
        assert np.array_equal(r["counters"], ref["counters"]), H
        for w in range(2):
            assert int(r["rng"][w][0]) == int(ref["rng"][w][0]) and np.array_equal(r["rng"][w][1], ref["rng"][w][1]), H
            assert np.array_equal(r["steps"][w], ref["steps"][w]), H


@pytest.mark.parametrize("name", ["c5_n256_aziz_s1982", "c5_n256_dipolar_s1982"])
@pytest.mark.parametrize("threads,split", [(None, 0), (256, 0), (None, 1)])
def test_k6_config5_n256_321_beads_worm_sector(gpu_lib, oracle, name, threads, split):
    r = run_k6(gpu_lib, oracle, [name], threads, split)
    assert r["drv"][0]["counters"][5] >= 1                  # the worm did open in the reference run
    worst, rel = check_against_driver(r, 0)
    print(f"{name}: worldline max |d| = {worst:.2e}, step energies max rel = {rel:.2e}")


@pytest.mark.parametrize("names", [["he4_wormbusy_s7", "he4_wormbusy_s8"],
                                   ["he4_worm_s1982", "he4_worm_s1983", "he4_worm_s1984"],
                                   ["he4_bis_cworm0_s1982", "he4_bis_cworm0_s1983"], ["he4_stock_short"],
                                   ["he4_wf_analytic"], ["he4_nlev1"]])
@pytest.mark.parametrize("split", [0, 1])
def test_k6_small_runs_full_state(gpu_lib, oracle, names, split):
    """The same full-state comparison on the small runs: dozens of accepted swaps, opens and closes, Npw = 1 and 2,
    and the analytic trial function (wf_table = F, the reference's default)."""
    r = run_k6(gpu_lib, oracle, names, split=split)
    for w in range(len(names)):
        check_against_driver(r, w)


# ---- long trajectories at the BASELINE sizes: past the cold start ------------------------------------------------------
LONG_FORMS = [(None, 0, None), (256, 0, 0), (None, 1, None), (None, 0, 0)]


def _check_block_checkpoints(r, w, upto=None):
    """driver.npz of the long runs holds the reference's state at the end of every block; the last one is the final state."""
    drv = r["drv"][w]
    assert np.array_equal(drv["ckpt_sha"][-1], drv["Path_sha256"]) and int(drv["ckpt_mti"][-1]) == int(drv["mti"])
    assert np.array_equal(drv["ckpt_counters"][-1], drv["counters"])


@pytest.mark.parametrize("threads,split,cm", LONG_FORMS)
def test_k6_config3_long_equilibrating_trajectory(gpu_lib, oracle, threads, split, cm):
    """C3 (N=256, 161 beads, stock schedule), 50 MC steps from the reference's init for seeds 1982 and 1983: 30 steps of
    warm-up during which acceptance and bead spread settle, then 20 in the regime bench.py times.  Every form of the
    sampler: generator state word for word, all counters, final worldline BIT-identical (SHA-256), every step's six
    energies to 1e-10."""
    names = ["c3_n256_long_s1982", "c3_n256_long_s1983"]
    r = run_k6(gpu_lib, oracle, names, threads, split, cm)
    for w in range(2):
        drv = r["drv"][w]
        assert len(drv["steps"]) == 50 and drv["counters"][3] > 20000       # bisection moves accepted: an equilibrating chain
        _check_block_checkpoints(r, w)
        worst, rel = check_against_driver(r, w)
        print(f"walker {w}: step energies max rel = {rel:.2e}")


@pytest.mark.parametrize("name", ["c5_n256_aziz_long_s1982", "c5_n256_dipolar_long_s1982"])
@pytest.mark.parametrize("threads,split,cm", LONG_FORMS)
def test_k6_config5_long_worm_trajectories(gpu_lib, oracle, name, threads, split, cm):
    """C5 (N=256, 321 beads, Npw = 2) with the STOCK CWorm = 0.5 for 60 MC steps.  Aziz table: 4 accepted opens and 4
    accepted closes; dipolar table: 1 open and > 100 accepted swaps (the reference accepts no swap with the Aziz table
    and no close with the dipolar one within 200 steps at this dt) -- every worm event at this size between the two.
    Event log identical in order and arguments, generator state, counters, bit-identical worldline and worm ends, OBDM
    histogram, energies of the diagonal steps."""
    r = run_k6(gpu_lib, oracle, [name], threads, split, cm)
    c = r["drv"][0]["counters"]
    if "aziz" in name:
        assert c[5] >= 3 and c[7] >= 3                      # accepted opens, closes
    else:
        assert c[5] >= 1 and c[13] >= 100                   # accepted opens, swaps
    _check_block_checkpoints(r, 0)
    worst, rel = check_against_driver(r, 0)
    print(f"{name}: step energies max rel = {rel:.2e}")
