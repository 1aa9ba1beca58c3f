"""The estimator files of the front end over several blocks, several steps per block and open walkers, against an
independent expectation: what pigs_vpi.f90 does with the accumulate kernels' sums -- which walkers it accumulates after
a step, the per-walker reset at the end of a block, the sample count it normalises by, the blocks it skips, the two
moments per walker, the all-reduced block vector and its counts, press_vpi.out and the shell files.

Method: replay through the API.  The front end dumps only the final worldline, so the worldline of every step comes
from a replay of the same chains through PigsContext (oracle.init_path with seed + w for walker w, sampler_set_rng,
upload_all, sampler_init with the input's parameters, one sampler_step per step; after each, download_all and the open
flags of sampler_get_worm), the way test_gpu_sampler.py drives the device sampler.  The device sampler, the host-driven
one and the reference are bit-identical (pinned elsewhere), so one replay serves device_sampler = T and F.  Every
scenario first asserts that the replay IS the run: its final worldlines have the bits of worldlines_final.bin, its
diagonal blocks are the rows of e_vpi.w####.out and its diagonal steps per block the run's "Diagonal conf." figure.

From the snapshots the raw sums of the diagonal walkers come from the numpy restatements that pin the kernels
(sqv_numpy, fqv_numpy, fqs_numpy, fqt_numpy, grv_numpy, tau_numpy, test_gpu_trap_profiles.ref_counts, and for the five
newer families bop_numpy, vh_numpy, g3_numpy, atm_numpy), and block_stats_numpy.py turns them into the files' columns.
momentum is the one exception: a step's end-to-end vectors live on the device tape, so its raw sums per step are what
pigs_nk_accumulate added during the replay (pinned against nk_numpy in test_gpu_nk.py); the rule by which a block
normalises n(k), the carry-over, zconf and the normalisation are restated here (momentum_blocks, block_stats_numpy).

The newer families where they meet the others: A+ (all ten periodic diagonal keys in one 3D run, single keys against
it), B+ and D+ (the worm run with all ten keys, unsharded and on two contexts: partial and empty blocks, momentum's own
block count next to the diagonal families' on one all-reduced vector), E (boxes with unequal sides, the box-dependent
defaults left out), L (lattice beside the ten periodic diagonal keys on he4_crystal, its raw sums from lat_numpy on the
replay's snapshots and its columns from block_stats_numpy.norm_lat), S (superfluid behind those eleven on the same run,
its raw sums from sf_numpy on the replay's snapshots and its columns from block_stats_numpy.norm_sf, per walker and
all-reduced).

Tolerances: the restatements' own per-element bounds, carried through the block sums, the normalisation and the means,
plus one unit of the tenth printed digit (PRINT); integer histograms: PRINT alone; error columns, the root of a
difference of two moments: sqrt(4 |mean| mtol) + PRINT |err| (test_gpu_fqt.py).  Where the expected error itself lies
below that allowance the error bar is ill-conditioned (the difference of the moments may round below zero: NaN); such
rows may be NaN, at most 1 % of a file's rows."""
import os
import re
import subprocess

import numpy as np
import pytest

import block_stats_numpy as bs
from conftest import GOLDEN, ROOT
from helpers import same_bits

RUNS = os.path.join(GOLDEN, "vpi_runs")
HOST = os.path.join(ROOT, "pathintegralgroundstate_amd", "host")
PRINT = 1.0000001e-9            # the files carry 10 significant digits
gpu = pytest.mark.gpu

# estimator grids: small, so that numpy stays fast
NMAX, WINDOW, NTAU, GR_NBIN = 2, 2, 3, 8
BO_NH, BO_NR, G3_NR, G3_NA, ATM_NU, NK_NMAX, NK_NBIN = 8, 8, 3, 4, 2.5, 2, 4
LAT_NBIN = 6
SF_NTAU = 3
# (the self part of van Hove at lag 0 is one full bin, the same value in every block: an ill-conditioned error bar by the
# expectation alone.  25 bins x 4 lags keep that one row within 1 % of the file's rows; bins of 0.08 resolve the displacements)
VH_NS, VH_RSELF = 25, 2.0
KEYS = {"fq_tau": f"fq_tau = T, fq_ntau = {NTAU}, fq_window = {WINDOW}",
        "sq_vector": f"sq_vector = T, sq_nmax = {NMAX}, sq_window = {WINDOW}",
        "fq_vector": f"fq_vector = T, fqv_nmax = {NMAX}, fqv_ntau = {NTAU}, fqv_window = {WINDOW}",
        "fq_self": f"fq_self = T, fqs_nmax = {NMAX}, fqs_ntau = {NTAU}, fqs_window = {WINDOW}",
        "gr_vector": f"gr_vector = T, gr_nbin = {GR_NBIN}, gr_window = {WINDOW}",
        "tau_profile": f"tau_profile = T, tau_window = {WINDOW}",
        "density_profile": "density_profile = T",
        # (RNB: bo_rnb(cfg), which _gpu_group fills in)
        "bond_order": f"bond_order = T, bo_rnb = RNB, bo_nhist = {BO_NH}, bo_nr = {BO_NR}, bo_window = {WINDOW}",
        "van_hove": f"van_hove = T, vh_ntau = {NTAU}, vh_window = {WINDOW}, vh_nself = {VH_NS}, vh_rself = {VH_RSELF!r}d0",
        "triplet": f"triplet = T, g3_nr = {G3_NR}, g3_na = {G3_NA}, g3_window = {WINDOW}",
        "three_body": f"three_body = T, atm_window = {WINDOW}, atm_nu = {ATM_NU!r}d0",
        "momentum": f"momentum = T, nk_nmax = {NK_NMAX}, nk_nbin = {NK_NBIN}",
        # (RMAX: the range of the displacement histograms, which scenario L fills in)
        "lattice": f"lattice = T, lat_window = {WINDOW}, lat_nbin = {LAT_NBIN}, lat_rmax = RMAX",
        # (fewer lags than the window of five slices holds)
        "superfluid": f"superfluid = T, sf_ntau = {SF_NTAU}, sf_window = {WINDOW}"}
FILES = {"fq_tau": ["fqt_vpi"], "sq_vector": ["sqvec_vpi", "sq_vpi"], "fq_vector": ["fqvec_vpi", "fqsh_vpi"],
         "fq_self": ["fqself_vpi", "fqssh_vpi", "msd_vpi"], "gr_vector": ["grvec_vpi", "grw_vpi"],
         "tau_profile": ["tau_vpi"], "density_profile": ["dens_vpi", "rho_vpi", "pr_vpi"],
         "bond_order": ["bo_vpi", "boh_vpi", "g6_vpi"], "van_hove": ["gd_vpi", "gs_vpi"], "triplet": ["g3_vpi", "g3ang_vpi"],
         "three_body": ["v3tau_vpi"], "momentum": ["nkvec_vpi", "nk_vpi", "nrvec_vpi"],
         "lattice": ["lind_vpi", "lindtau_vpi", "usite_vpi"], "superfluid": ["rhos_vpi", "msdu_vpi"]}
# the files with one line per block, which check_v3 and check_n0 read
BLOCK_FILES = {"tau_profile": ["press_vpi"], "three_body": ["v3_vpi"], "momentum": ["n0_vpi"]}
# scenario B: (Nblock, Nstep) of he4_wormbusy_s7 with four walkers, chosen from the replay's open / closed pattern over 60
# steps.  Diagonal steps per block: walker 0: 1 0 0 0 0 0 0 0, walker 1: 5 0 0 1 5 2 3 6, walker 2: 6 3 0 0 0 2 6 3,
# walker 3: 3 0 0 0 5 6 0 0 -- empty blocks before counted ones, partial blocks, and block 3 diagonal for nobody
B_BLOCKS, B_STEPS, B_WALKERS = 8, 6, 4


# ---- the helper itself, on synthetic block values (no GPU) ------------------------------------------------------------
def test_block_statistics_helper_against_hand_written_moments():
    """Three walkers, four blocks: walker 0 counts all of them, walker 1 misses block 1, walker 2 counts block 2 only.
    Against the two-moment formulas written out by hand."""
    b = np.array([[1.0, 2.0, 4.0, 8.0], [3.0, 100.0, 5.0, 9.0], [-50.0, -60.0, 7.0, -70.0]])[:, :, None] * np.array([1.0, -2.0])
    counted = np.array([[1, 1, 1, 1], [1, 0, 1, 1], [0, 0, 1, 0]], bool)
    m, e, n = bs.walker_stats(b, counted, 0)
    assert n == 4 and np.allclose(m, [3.75, -7.5], rtol=1e-15)
    assert np.allclose(e[0], np.sqrt(((1 + 4 + 16 + 64) / 4.0 - 3.75 ** 2) / 4.0), rtol=1e-14) and np.allclose(e[1], 2 * e[0], rtol=1e-14)
    m, e, n = bs.walker_stats(b, counted, 1)                           # the uncounted block's 100 must not show
    assert n == 3 and np.allclose(m[0], 17.0 / 3.0, rtol=1e-15)
    assert np.allclose(e[0], np.sqrt(((9 + 25 + 81) / 3.0 - (17.0 / 3.0) ** 2) / 3.0), rtol=1e-13)
    m, e, n = bs.walker_stats(b, counted, 2)                           # a single counted block: its value, error 0
    assert n == 1 and m[0] == 7.0 and e[0] == 0.0
    av, cb = bs.walker_average(b, counted)
    assert cb.tolist() == [True] * 4                                   # unequal counts: 2, 1, 3, 2 walkers
    assert np.allclose(av[:, 0], [(1 + 3) / 2.0, 2.0, (4 + 5 + 7) / 3.0, (8 + 9) / 2.0], rtol=1e-15)
    m, e, n = bs.average_stats(b, counted)
    x = np.array([2.0, 2.0, 16.0 / 3.0, 8.5])
    assert n == 4 and np.allclose(m[0], x.sum() / 4, rtol=1e-15)
    assert np.allclose(e[0], np.sqrt(((x * x).sum() / 4 - (x.sum() / 4) ** 2) / 4), rtol=1e-13)
    # a block that nobody counted is no block of the averaged file; a walker that never counted gives NaN
    counted[:, 3] = False
    m, e, n = bs.average_stats(b, counted)
    assert n == 3 and np.allclose(m[0], x[:3].sum() / 3, rtol=1e-15)
    m, e, n = bs.walker_stats(b, np.zeros((3, 4), bool), 0)
    assert n == 0 and np.all(np.isnan(m)) and np.all(np.isnan(e))
    assert np.allclose(bs.mean_bound(np.abs(b), counted, 1)[0], (3.0 + 5.0) / 2.0, rtol=1e-15)
    # the normalisations, on numbers small enough to divide by hand
    assert bs.norm_window([[30.0]], [2], 3, 2)[0, 0] == 30.0 / (2 * 5 * 3)
    assert np.allclose(bs.norm_lags(np.full((1, 3, 2), 60.0), [2], 3, 1, -2)[0, :, 0], [60 / 18.0, 60 / 12.0, 60 / 6.0], rtol=1e-15)
    T = bs.norm_tau(np.array([[[4.0, 0.0, 8.0, 0.02]] * 3]), [2], 2, 3, 0.1)
    assert np.allclose(T[0, 0], [1.0, 0.0, 2.0, 15.0 - 0.02 / (2 * 0.01 * 2 * 2)], rtol=1e-15) and T[0, 2, 3] == 0.0
    assert bs.pressure(3.0, 1.0, 0.5, 2) == 0.25 * 5.0
    idx, q, mult = bs.shells(np.array([[0, 0, 1], [0, 1, 0], [0, 1, 1], [1, 0, 0]]), [2.0, 2.0, 2.0])
    assert idx.tolist() == [0, 0, 1, 0] and mult.tolist() == [6, 2] and np.allclose(q, [np.pi, np.pi * np.sqrt(2.0)], rtol=1e-15)
    assert np.allclose(bs.shell_means(idx, 2, np.array([1.0, 2.0, 10.0, 6.0])), [3.0, 10.0], rtol=1e-15)
    # the five newer families.  Bond order: S = 2 samples of window 1, n = 6 slices, Np = 4
    B, P, G6 = bs.norm_bop([3.0, 9.0, 1.5, 9.0, 2.4, 1.2, 48.0, 0.0], [[12, 0, 12], [24, 0, 0]], [1.0, 0.0, -3.0], [4, 0, 2], 2, 4, 1)
    assert np.allclose(B, [0.5, 0.25, 0.4, 0.2, 2.0], rtol=1e-15) and G6.tolist() == [0.25, 0.0, -1.5]
    assert np.allclose(P, [[1.5, 0.0, 1.5], [3.0, 0.0, 0.0]], rtol=1e-15) and np.allclose(P.sum(axis=1) / 3.0, 1.0, rtol=1e-15)
    # van Hove in 2D: shells pi b^2 (1, 3); S = 2, window 1, lags 0, 1 with 3 and 2 slice pairs, Np = 5, density 0.5
    gs, gd = bs.norm_vh([[30, 90], [20, 0]], [[60, 0], [0, 120]], 2, 5, 1, 0.5, 2.0, 1.0, 2)
    assert np.allclose(gs, [[1 / np.pi, 1 / np.pi], [1 / np.pi, 0.0]], rtol=1e-15)
    assert np.allclose(gd, [[1 / np.pi, 0.0], [0.0, 1 / np.pi]], rtol=1e-15)
    # triplets in 3D: Nr = 2, rbin 1: shells 4 pi/3 (1, 7); packed (0,0), (0,1), (1,1); Na = 2; n = 2 slices, Np = 3, density 0.5
    v = 4.0 * np.pi / 3.0
    g2, g3, pa = bs.norm_g3([[3, 0], [0, 21], [49, 49]], [3, 21], 2, 3, 0, 0.5, 1.0, 3)
    assert np.allclose(g2, [1 / v, 1 / v], rtol=1e-15)
    assert np.allclose(g3, np.array([[8.0, 0.0], [0.0, 4.0], [8 / 3.0, 8 / 3.0]]) / (v * v), rtol=1e-15)
    assert np.allclose(pa, [52 / 122.0, 70 / 122.0], rtol=1e-15) and not bs.norm_g3(np.zeros((3, 2)), [0, 0], 2, 3, 0, 0.5, 1.0, 3)[2].any()
    # ... and the angle weights in 2D: cos(theta) in [-1, 0) and [0, 1) hold half of the angles each, four bins 1/3, 1/6, 1/6, 1/3
    g3 = bs.norm_g3(np.ones((1, 4)), [1], 1, 1, 0, 1.0, 1.0, 2)[1]
    assert np.allclose(g3[0], 2.0 / (np.pi ** 2 * np.array([1 / 3.0, 1 / 6.0, 1 / 6.0, 1 / 3.0])), rtol=1e-14)
    v3, nt, win, p3 = bs.norm_atm([6.0, -3.0, 12.0], [4, 0, 2], 2, 3, 2.5, 0.4, 3)
    assert np.allclose(v3, [2.5, -1.25, 5.0], rtol=1e-15) and nt.tolist() == [2.0, 0.0, 1.0]
    assert np.allclose([win, p3], [6.25 / 3.0, 9 * 0.4 * (6.25 / 3.0) / 3.0], rtol=1e-15)
    nk, n0 = bs.norm_nk([6.0, -3.0], 12, 0.5, 6, 4, 8)
    assert nk.tolist() == [1.0, 0.5, -0.25] and n0 == 0.125
    assert bs.norm_nrvec([[12, 0], [0, 6]], 0.5, 6, 4, 0.25, [2.0, 4.0], 2).tolist() == [[2.0, 0.0], [0.0, 1.0]]


# ---- running and replaying ----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def exe(gpu_lib):
    subprocess.check_call(["make", "-s", "-C", HOST])
    return os.path.join(HOST, "pigs_vpi")


def _run(exe, txt, wd, timeout=300):
    """One front-end run in a fresh child process under its own time limit; a non-zero exit fails the test at once."""
    os.makedirs(wd, exist_ok=True)
    with open(os.path.join(wd, "vpi.in"), "w") as f:
        f.write(txt)
    with open(os.path.join(wd, "vpi.in")) as fin, open(os.path.join(wd, "stdout.txt"), "w") as fo:
        r = subprocess.run([exe], stdin=fin, stdout=fo, stderr=subprocess.STDOUT, cwd=wd, timeout=timeout)
    out = open(os.path.join(wd, "stdout.txt")).read()
    assert r.returncode == 0, out[-3000:]
    return out


def _input(name, Nblock, Nstep):
    from pathintegralgroundstate_amd import SystemConfig
    txt = open(os.path.join(RUNS, name, "vpi.in")).read()
    txt, k1 = re.subn(r"Nblock\s*=\s*\d+", f"Nblock = {Nblock}", txt)
    txt, k2 = re.subn(r"Nstep\s*=\s*\d+", f"Nstep = {Nstep}", txt)
    assert k1 == 1 and k2 == 1
    return txt, SystemConfig.from_namelists(txt)


def bo_rnb(cfg):
    """The first-shell radius of test_gpu_bop.py: the ball that holds 12 (3D) or 6 (2D) particles at the run's density, at
    most half the shortest side; cut to six decimals, which the namelist and numpy then read as the same double."""
    r = (6.0 / (np.pi * cfg.density)) ** 0.5 if cfg.dim == 2 else (36.0 / (4.0 * np.pi * cfg.density)) ** (1.0 / 3.0)
    return np.floor(min(r, cfg.rcut) * 1e6) / 1e6


def _gpu_group(keys, W, extra="", cfg=None):
    txt = f"&gpu\n n_walkers = {W}, {extra}" + ", ".join(KEYS[k] for k in keys) + "\n/\n"
    return txt.replace("RNB", f"{bo_rnb(cfg):.6f}d0") if "bond_order" in keys else txt


def replay(gpu_lib, oracle, cfg, W, Nblock, Nstep, nk=None, start=None):
    """The run's chains through the API: the worldlines after every step [T, W, M, Np, dim], whether each walker is in the
    diagonal sector after it [T, W], and the final worldlines.  nk = (nmax, nbin): the momentum sums as well, which live
    on the device tape of a step's worm loops and in no snapshot: nk_accumulate after every step, and under "nk" per step
    what the step added to C, H and nopen (the difference of two reads without reset), with the stored vectors n, and
    under "zdiag" sampler_events()[:, 1] == 0 per step, what the front end counts its diagonal configurations by.
    start [Np, dim]: the positions of a lattice start (crystal = T), which every walker begins on with a freshly seeded
    generator."""
    from oracle.pyoracle import System
    S = System(dim=cfg.dim, Np=cfg.Np, Nb=cfg.Nb, density=cfg.density, dt=cfg.dt, trap=cfg.trap, a_ho=cfg.a_ho,
               Lbox=cfg.Lbox, rcut=cfg.rcut)
    VT, WF = gpu_lib.build_tables(cfg)
    snaps, diag = [], []
    with gpu_lib.PigsContext(cfg, VT, WF, n_walkers=W) as ctx:
        ctx.sampler_init(CWorm=cfg.CWorm, swapping=cfg.swapping, Nobdm=cfg.Nobdm, Nbin=cfg.Nbin, Npw=cfg.Npw,
                         sampling=cfg.sampling)
        P0, xend = [], []
        for w in range(W):
            P, g = oracle.init_path(S, cfg.seed + w)                   # pigs_vpi.f90: walker w runs the chain of seed + w
            if start is not None:
                P, g = np.broadcast_to(start, tuple(cfg.path_shape)).copy(), oracle.rng(cfg.seed + w)
            P0.append(P)
            xend.append(np.stack([P[cfg.Nb, cfg.Np - 1], P[cfg.Nb, cfg.Np - 1]]))
            ctx.sampler_set_rng(w, g.mti, np.array(g.mt[:], np.uint32))
        ctx.upload_all(np.stack(P0))
        ctx.sampler_set_worm(np.zeros(W, np.int32), np.zeros(W, np.int32), np.stack(xend))
        inc, zdiag = {"C": [], "H": [], "nopen": []}, []
        if nk is not None:
            ctx.nk_init(*nk)
            last = ctx.nk_read()
        for _ in range(Nblock):
            for istep in range(1, Nstep + 1):
                ctx.sampler_step(istep)
                if nk is not None:
                    ctx.nk_accumulate()
                    now = ctx.nk_read()
                    for k in inc:
                        inc[k].append(now[k] - last[k])
                    last = now
                    zdiag.append(ctx.sampler_events()[:, 1] == 0)
                snaps.append(ctx.download_all())
                diag.append(~ctx.sampler_get_worm()[0])
        final = ctx.download_all()
        extra = {}
        if nk is not None:
            extra = {"nk": dict({k: np.stack(v) for k, v in inc.items()}, n=ctx.nk_vectors()), "zdiag": np.stack(zdiag)}
    return dict(snaps=np.stack(snaps), diag=np.stack(diag), final=final, VT=VT, W=W, Nblock=Nblock, Nstep=Nstep, cfg=cfg, **extra)


def _blocks(x, rep):
    """Per-step sums [T, W, ...] -> per-block sums [W, Nblock, ...]."""
    x = np.asarray(x)
    return np.moveaxis(x.reshape((rep["Nblock"], rep["Nstep"]) + x.shape[1:]).sum(axis=1), 0, 1)


def family_grids(cfg, **over):
    """The grids of the five newer families as the run sets them up: KEYS' values, and for what a run leaves out the
    defaults that the front end's header documents (half the shortest side, rcut, the run's g(r) grid)."""
    g = dict(rnb=bo_rnb(cfg), bo_nh=BO_NH, bo_nr=BO_NR, vh_ns=VH_NS, vh_rself=VH_RSELF, g3_nr=G3_NR, g3_na=G3_NA,
             g3_rmax=0.5 * min(cfg.Lbox[:cfg.dim]), atm_rc=0.5 * min(cfg.Lbox[:cfg.dim]), atm_nu=ATM_NU)
    g.update(over)
    g["bo_rbin"] = cfg.rbin if g["bo_nr"] == cfg.Nbin else cfg.rcut / g["bo_nr"]
    g["vh_sbin"], g["g3_rbin"] = g["vh_rself"] / g["vh_ns"], g["g3_rmax"] / g["g3_nr"]
    return g


def momentum_blocks(zdiag_blocks, Nstep):
    """The front end's rule for the blocks that normalise n(k), restated: a walker counts its diagonal configurations
    since its last normalised block, and a block normalises once they are Nstep or more, with that count as zconf; the
    sums of the blocks before it are carried over.  zdiag_blocks [W, Nblock] -> (norm [W, Nblock] bool, zconf, first):
    first [W, Nblock] the first block whose sums a normalising block holds."""
    W, nb = zdiag_blocks.shape
    norm, zconf, first = np.zeros((W, nb), bool), np.zeros((W, nb), np.int64), np.zeros((W, nb), np.int64)
    for w in range(W):
        aux, start = 0, 0
        for b in range(nb):
            aux += int(zdiag_blocks[w, b])
            first[w, b] = start
            if aux >= Nstep:
                norm[w, b], zconf[w, b] = True, aux
                aux, start = 0, b + 1
    return norm, zconf, first


def expectation(rep, keys, **grids):
    """Block values and their bounds per file, from the replay: {file base: (values [W, Nblock, ...], bound or None)},
    plus "counted" [W, Nblock], "samples" and the raw block sums under "raw".  momentum's files are normalised in blocks
    of their own: "counted_of" holds their mask per file."""
    import atm_numpy
    import bop_numpy
    import g3_numpy
    import vh_numpy
    import fqs_numpy
    import fqt_numpy
    import fqv_numpy
    import grv_numpy
    import sqv_numpy
    import tau_numpy
    from test_gpu_trap_profiles import ref_counts
    cfg, snaps, diag, W = rep["cfg"], rep["snaps"], rep["diag"], rep["W"]
    T = snaps.shape[0]
    dim, Np, Nb, L = cfg.dim, cfg.Np, cfg.Nb, cfg.Lbox
    S = _blocks(diag.astype(np.int64), rep)                            # samples [W, Nblock]
    E = {"samples": S, "counted": S > 0, "raw": {}, "counted_of": {}}
    steps = {}
    gd = E["grid"] = family_grids(cfg, **grids)
    ns = 2 * WINDOW + 1

    def add(name, t, val):
        steps.setdefault(name, [None] * T)[t] = val

    n = sqv_numpy.vectors(dim, NMAX) if not cfg.trap else None
    for t in range(T):
        ws = [int(w) for w in np.flatnonzero(diag[t])]                 # the diagonal walkers of the step, nobody else
        P = snaps[t]
        if "fq_tau" in keys:
            F, B, _ = fqt_numpy.expected(P, ws, Nb, WINDOW, NTAU, cfg.Nk, L)
            add("fqt", t, F), add("fqt_b", t, B)
        if "sq_vector" in keys:
            A, B, _ = sqv_numpy.expected(P, ws, Nb, WINDOW, n, L)
            add("sqv", t, A), add("sqv_b", t, B)
        if "fq_vector" in keys:
            A, B, _ = fqv_numpy.expected(P, ws, Nb, WINDOW, NTAU, n, L)
            add("fqv", t, A), add("fqv_b", t, B)
        if "fq_self" in keys:
            e = fqs_numpy.expected(P, ws, Nb, WINDOW, NTAU, n, L)
            add("fqs", t, e["F"]), add("fqs_b", t, e["Fb"]), add("msd", t, e["D"]), add("msd_b", t, e["Db"])
        if "gr_vector" in keys:
            V, R, _, dropped = grv_numpy.expected(P, ws, Nb, WINDOW, L, cfg.rcut2, GR_NBIN, cfg.Nbin, cfg.rbin)
            assert dropped == 0
            add("grv", t, V), add("grw", t, R)
        if "tau_profile" in keys:
            Q, A, _ = tau_numpy.expected(P, ws, rep["VT"], cfg)
            add("tau", t, Q), add("tau_b", t, A)
        if "density_profile" in keys:
            h = cfg.rcut / 2.0
            c = [np.zeros((W, cfg.Nbin ** min(dim, 2)), np.int64), np.zeros((W, cfg.Nbin), np.int64), np.zeros((W, cfg.Nbin), np.int64)]
            for w in ws:
                for a, x in zip(c, ref_counts(P[w, Nb], cfg.Nbin, h)):
                    a[w] = x
            add("dpl", t, c[0]), add("drad", t, c[1]), add("dpair", t, c[2])
        if "bond_order" in keys:
            e = bop_numpy.Window(P, L, cfg.rcut2, gd["rnb"]).expected(ws, Nb, WINDOW, gd["bo_nr"], gd["bo_rbin"])
            H = np.zeros((W, 2, gd["bo_nh"]), np.int64)
            B = np.zeros((W, 8))                                       # test_gpu_bop.py's bounds on S, element for element
            for w in ws:
                H[w] = [bop_numpy.histogram(np.concatenate(e[k][w]), gd["bo_nh"]) for k in ("q4", "q6")]
                B[w] = [sum(1e-12 / max(Q, 1e-6) for Q in e["Q4"][w]), 1e-12 * ns, sum(1e-12 / max(Q, 1e-6) for Q in e["Q6"][w]),
                        1e-12 * ns, 1e-12 * ns, 1e-12 * ns, 0.0, 0.0]
            add("boS", t, e["S"]), add("boS_b", t, B), add("boH", t, H), add("boG", t, e["G"]), add("boGN", t, e["GN"])
        if "van_hove" in keys:
            e = vh_numpy.expected(P, ws, Nb, WINDOW, NTAU, L, cfg.rcut2, cfg.Nbin, cfg.rbin, gd["vh_ns"], gd["vh_sbin"])
            add("vhs", t, e["self"]), add("vhd", t, e["distinct"])
        if "triplet" in keys:
            e = g3_numpy.Window(P, Nb, WINDOW, L).expected(ws, gd["g3_nr"], gd["g3_rbin"], gd["g3_na"])
            add("g3t", t, e["trip"]), add("g3p", t, e["pair"])
        if "three_body" in keys:
            e = atm_numpy.Window(P, Nb, WINDOW, L).expected(ws, gd["atm_rc"])
            add("atm", t, e["T"]), add("atm_b", t, 1e-12 * e["abs"]), add("atm_n", t, e["ntrip"])      # test_gpu_atm.py's bound
    raw = E["raw"] = {k: _blocks(np.stack(v), rep) for k, v in steps.items()}
    cnt = E["counted"]

    def clean(x):
        """Block values of the counted blocks; zeros where the walker had no sample (0 / 0 otherwise)."""
        x = np.array(x, np.float64)
        x[~cnt] = 0.0
        return x

    if "fq_tau" in keys:
        E["fqt_vpi"] = (clean(bs.norm_lags(raw["fqt"], S, Np, WINDOW, -3)), clean(bs.norm_lags(raw["fqt_b"], S, Np, WINDOW, -3)))
    if not cfg.trap and {"sq_vector", "fq_vector", "fq_self"} & set(keys):
        idx, q, mult = bs.shells(n, L)
        E["shells"] = (idx, q, mult)
    if "sq_vector" in keys:
        v, b = clean(bs.norm_window(raw["sqv"], S, Np, WINDOW)), clean(bs.norm_window(raw["sqv_b"], S, Np, WINDOW))
        E["sqvec_vpi"] = (v, b)
        E["sq_vpi"] = (bs.shell_means(idx, q.size, v), bs.shell_means(idx, q.size, b))
    for key, name, vec, sh in (("fq_vector", "fqv", "fqvec_vpi", "fqsh_vpi"), ("fq_self", "fqs", "fqself_vpi", "fqssh_vpi")):
        if key in keys:
            v, b = clean(bs.norm_lags(raw[name], S, Np, WINDOW, -2)), clean(bs.norm_lags(raw[name + "_b"], S, Np, WINDOW, -2))
            E[vec] = (v, b)
            E[sh] = (bs.shell_means(idx, q.size, v), bs.shell_means(idx, q.size, b))
    if "fq_self" in keys:
        E["msd_vpi"] = (clean(bs.norm_lags(raw["msd"], S, Np, WINDOW, -2)), clean(bs.norm_lags(raw["msd_b"], S, Np, WINDOW, -2)))
    if "gr_vector" in keys:
        gv, gr = bs.norm_grv(raw["grv"], raw["grw"], S, Np, WINDOW, cfg.density, L, cfg.rbin, dim)
        E["grvec_vpi"] = (clean(gv).reshape(W, rep["Nblock"], -1), None)        # x fastest: the last axis
        E["grw_vpi"] = (clean(gr), None)
    if "tau_profile" in keys:
        Tq = clean(bs.norm_tau(raw["tau"], S, Np, dim, cfg.dt))
        with np.errstate(all="ignore"):
            Tb = 1e-12 * raw["tau_b"] / (S[:, :, None, None] * Np)
            Tb[..., 3] = 1e-12 * raw["tau_b"][..., 3] / (2.0 * cfg.dt ** 2 * Np * S[:, :, None]) + 4e-16 * dim / (2.0 * cfg.dt)
        E["tau_vpi"] = (Tq, clean(Tb))
    if "density_profile" in keys:
        a, b, c = bs.norm_density(raw["dpl"], raw["drad"], raw["dpair"], S, dim, Np, cfg.Nbin, cfg.rcut / 2.0)
        E["dens_vpi"], E["rho_vpi"], E["pr_vpi"] = (clean(a), None), (clean(b), None), (clean(c), None)
    nbl = rep["Nblock"]
    if "bond_order" in keys:
        b, p, g6 = bs.norm_bop(raw["boS"], raw["boH"], raw["boG"], raw["boGN"], S, Np, WINDOW)
        bb = bs.norm_bop(raw["boS_b"], raw["boH"], raw["boG"], raw["boGN"], S, Np, WINDOW)[0]
        E["bo_vpi"] = (clean(b), clean(bb))
        E["boh_vpi"] = (clean(p), None)
        # (G within GN (1e-12 + 2^-41) in every bin, test_gpu_bop.py: G6 = G / GN within 1e-12 + 2^-41)
        E["g6_vpi"] = (clean(g6), clean(np.where(raw["boGN"] > 0, 1e-12 + 2.0 ** -41, 0.0)))
    if "van_hove" in keys:
        gs, gdist = bs.norm_vh(raw["vhs"], raw["vhd"], S, Np, WINDOW, cfg.density, cfg.rbin, gd["vh_sbin"], dim)
        E["gs_vpi"], E["gd_vpi"] = (clean(gs), None), (clean(gdist), None)
    if "triplet" in keys:
        _, g3, pang = bs.norm_g3(raw["g3t"], raw["g3p"], S, Np, WINDOW, cfg.density, gd["g3_rbin"], dim)
        E["g3_vpi"], E["g3ang_vpi"] = (clean(g3), None), (clean(pang), None)
    if "three_body" in keys:
        v3, nt, win, p3 = bs.norm_atm(raw["atm"], raw["atm_n"], S, Np, gd["atm_nu"], cfg.density, dim)
        v3b, _, winb, _ = bs.norm_atm(raw["atm_b"], raw["atm_n"], S, Np, abs(gd["atm_nu"]), cfg.density, dim)
        E["v3tau_vpi"] = (clean(v3), clean(v3b))
        E["v3_ntrip"], E["v3_vpi"] = clean(nt), (clean(win), clean(winb))
    if "momentum" in keys:
        nk, Nstep = rep["nk"], rep["Nstep"]
        assert np.array_equal(nk["n"], sqv_numpy.vectors(dim, NK_NMAX))
        norm, zconf, first = momentum_blocks(_blocks(rep["zdiag"].astype(np.int64), rep), Nstep)
        Cb, Hb, nob = _blocks(nk["C"], rep), _blocks(nk["H"], rep).reshape(W, nbl, -1), _blocks(nk["nopen"], rep)
        vec, vecb = np.zeros((W, nbl, Cb.shape[-1] + 1)), np.zeros((W, nbl, Cb.shape[-1] + 1))
        rho, n0 = np.zeros((W, nbl, Hb.shape[-1])), np.zeros((W, nbl))
        raw["nkC"], raw["nkH"], raw["nkno"] = np.zeros(Cb.shape), np.zeros(Hb.shape, np.int64), np.zeros((W, nbl), np.int64)
        for w, b in zip(*np.nonzero(norm)):
            lo, z = first[w, b], float(zconf[w, b])
            C, H, no = Cb[w, lo:b + 1].sum(axis=0), Hb[w, lo:b + 1].sum(axis=0), nob[w, lo:b + 1].sum()
            raw["nkC"][w, b], raw["nkH"][w, b], raw["nkno"][w, b] = C, H, no
            vec[w, b], n0[w, b] = bs.norm_nk(C, no, cfg.CWorm, z, cfg.Nobdm, Np)
            # (C within 1e-12 of its number of samples, test_gpu_nk.py; the k = 0 line is a count)
            vecb[w, b, 1:] = 1e-12 * no / (cfg.CWorm * z * cfg.Nobdm)
            rho[w, b] = bs.norm_nrvec(H.reshape((NK_NBIN,) * dim), cfg.CWorm, z, cfg.Nobdm, cfg.density, L, dim).ravel()
        E["nkvec_vpi"], E["nrvec_vpi"] = (vec, vecb), (rho, None)
        if len(set(L[:dim])) == 1:                                     # (bs.shells: equal sides only)
            idk, qk, _ = E["nk_shells"] = bs.shells(nk["n"], L)
            E["nk_vpi"] = (bs.shell_means(idk, qk.size, vec[..., 1:]), bs.shell_means(idk, qk.size, vecb[..., 1:]))
        E["n0"], E["zconf"] = n0, zconf
        for base in FILES["momentum"] + ["n0_vpi"]:
            E["counted_of"][base] = norm
    return E


# ---- reading the files --------------------------------------------------------------------------------------------------
def _rows(path):
    return [[float(t) for t in ln.split()] for ln in open(path) if ln.strip() and not ln.startswith("#")]


def _table(path, shape):
    tab = np.array(_rows(path))
    assert tab.shape == shape, (path, tab.shape, shape)
    return tab


def read_file(d, base, suffix, rep, E):
    """(mean, err) of one file, shaped like the expectation's block values; the index columns are checked here: integer
    ones exactly, the printed reals to the printed digits."""
    cfg = rep["cfg"]
    dim, Nb, dt, L = cfg.dim, cfg.Nb, cfg.dt, np.asarray(cfg.Lbox[:cfg.dim])
    path = os.path.join(d, base + suffix + ".out")
    close = lambda a, b: np.allclose(a, b, rtol=PRINT, atol=0)
    nl = NTAU + 1
    if base == "fqt_vpi":
        tab = _table(path, (nl * cfg.Nk, 3 * dim))
        q = np.arange(1, cfg.Nk + 1)[:, None] * (2 * np.pi / L)[None, :]
        assert close(tab[:, 0::3], np.tile(q, (nl, 1)))
        hdr = [ln.split() for ln in open(path) if ln.startswith("#")]
        assert [(int(h[3]), int(h[9])) for h in hdr] == [(l, 2 * WINDOW + 1 - l) for l in range(nl)]
        assert close([float(h[6]) for h in hdr], np.arange(nl) * dt)
        return tab[:, 1::3].reshape(nl, cfg.Nk, dim), tab[:, 2::3].reshape(nl, cfg.Nk, dim)
    if base in ("sqvec_vpi", "fqvec_vpi", "fqself_vpi", "sq_vpi", "fqsh_vpi", "fqssh_vpi"):
        import sqv_numpy
        n = sqv_numpy.vectors(dim, NMAX)
        idx, qsh, mult = E["shells"]
        qmod = np.sqrt(((n * (2 * np.pi / L)) ** 2).sum(axis=1))
        if base == "sqvec_vpi":
            tab = _table(path, (n.shape[0], dim + 3))
            assert np.array_equal(tab[:, :dim], n) and close(tab[:, dim], qmod)
            return tab[:, dim + 1], tab[:, dim + 2]
        if base == "sq_vpi":
            tab = _table(path, (qsh.size, 4))
            assert close(tab[:, 0], qsh) and np.array_equal(tab[:, 3], mult)
            return tab[:, 1], tab[:, 2]
        if base in ("fqvec_vpi", "fqself_vpi"):
            Nq = n.shape[0]
            tab = _table(path, (nl * Nq, dim + 5))
            assert np.array_equal(tab[:, 0], np.repeat(np.arange(nl), Nq)) and close(tab[:, 1], tab[:, 0] * dt)
            assert np.array_equal(tab[:, 2:2 + dim], np.tile(n, (nl, 1))) and close(tab[:, 2 + dim], np.tile(qmod, nl))
            return tab[:, 3 + dim].reshape(nl, Nq), tab[:, 4 + dim].reshape(nl, Nq)
        tab = _table(path, (nl * qsh.size, 6))
        assert np.array_equal(tab[:, 0], np.repeat(np.arange(nl), qsh.size)) and close(tab[:, 1], tab[:, 0] * dt)
        assert close(tab[:, 2], np.tile(qsh, nl)) and np.array_equal(tab[:, 5], np.tile(mult, nl))
        return tab[:, 3].reshape(nl, qsh.size), tab[:, 4].reshape(nl, qsh.size)
    if base == "msd_vpi":
        tab = _table(path, (nl, 5))
        assert np.array_equal(tab[:, 0], np.arange(nl)) and close(tab[:, 1], np.arange(nl) * dt)
        return tab[:, 2:3], tab[:, 3:4], tab[:, 4]                     # (<dr^2> only; alpha_2 for its own check)
    if base == "grvec_vpi":
        tab = _table(path, (GR_NBIN ** dim, dim + 2))
        j = np.arange(GR_NBIN ** dim)
        for k in range(dim):
            x = -0.5 * L[k] + ((j // GR_NBIN ** k) % GR_NBIN + 0.5) * (L[k] / GR_NBIN)
            assert np.allclose(tab[:, k], x, rtol=PRINT, atol=PRINT * L[k])
        return tab[:, dim], tab[:, dim + 1]
    if base in ("grw_vpi", "rho_vpi", "pr_vpi"):
        tab = _table(path, (cfg.Nbin, 3))
        width = cfg.rbin if base == "grw_vpi" else cfg.rcut / 2.0 / cfg.Nbin
        assert close(tab[:, 0], (np.arange(cfg.Nbin) + 0.5) * width)
        return tab[:, 1], tab[:, 2]
    if base == "dens_vpi":
        assert dim == 2
        tab = _table(path, (cfg.Nbin ** 2, 4))
        h = cfg.rcut / 2.0
        x = -h + (np.arange(cfg.Nbin) + 0.5) * (2.0 * h / cfg.Nbin)
        assert np.allclose(tab[:, 0], np.tile(x, cfg.Nbin), rtol=PRINT, atol=PRINT * h)        # x fastest
        assert np.allclose(tab[:, 1], np.repeat(x, cfg.Nbin), rtol=PRINT, atol=PRINT * h)
        return tab[:, 2], tab[:, 3]
    gd = E["grid"]
    centres = lambda nb, width: (np.arange(nb) + 0.5) * width
    if base == "bo_vpi":
        tab = _table(path, (1, 10))
        return tab[0, 0::2], tab[0, 1::2]
    if base == "boh_vpi":
        tab = _table(path, (gd["bo_nh"], 5))
        assert close(tab[:, 0], centres(gd["bo_nh"], 1.0 / gd["bo_nh"]))
        return tab[:, 1::2].T, tab[:, 2::2].T                           # [2, Nh]: q4's distribution, then q6's
    if base == "g6_vpi":
        tab = _table(path, (gd["bo_nr"], 3))
        assert close(tab[:, 0], centres(gd["bo_nr"], gd["bo_rbin"]))
        return tab[:, 1], tab[:, 2]
    if base in ("gd_vpi", "gs_vpi"):
        nb, width = (cfg.Nbin, cfg.rbin) if base == "gd_vpi" else (gd["vh_ns"], gd["vh_sbin"])
        tab = _table(path, (nl * nb, 4))
        assert close(tab[:, 0], np.repeat(np.arange(nl) * dt, nb)) and close(tab[:, 1], np.tile(centres(nb, width), nl))
        return tab[:, 2].reshape(nl, nb), tab[:, 3].reshape(nl, nb)
    if base == "g3_vpi":
        Nr, Na = gd["g3_nr"], gd["g3_na"]
        lo, hi = np.triu_indices(Nr)                                   # the packed triangle: rows lo, hi = lo .. Nr - 1
        tab = _table(path, (lo.size * Na, 5))
        r = centres(Nr, gd["g3_rbin"])
        assert close(tab[:, 0], np.repeat(r[lo], Na)) and close(tab[:, 1], np.repeat(r[hi], Na))
        assert close(tab[:, 2], np.tile(-1.0 + centres(Na, 2.0 / Na), lo.size))
        return tab[:, 3].reshape(lo.size, Na), tab[:, 4].reshape(lo.size, Na)
    if base == "g3ang_vpi":
        tab = _table(path, (gd["g3_na"], 3))
        assert close(tab[:, 0], -1.0 + centres(gd["g3_na"], 2.0 / gd["g3_na"]))
        return tab[:, 1], tab[:, 2]
    if base == "v3tau_vpi":
        tab = _table(path, (2 * WINDOW + 1, 5))
        a = np.arange(Nb - WINDOW, Nb + WINDOW + 1)
        assert np.array_equal(tab[:, 0], a) and close(tab[:, 1], (a - Nb) * dt)
        return tab[:, 2], tab[:, 3], tab[:, 4]                         # (the mean number of triplets for its own check)
    if base == "nkvec_vpi":
        import sqv_numpy
        n = sqv_numpy.vectors(dim, NK_NMAX)
        tab = _table(path, (n.shape[0] + 1, dim + 3))
        assert not tab[0, :dim + 1].any() and np.array_equal(tab[1:, :dim], n)
        assert close(tab[1:, dim], np.sqrt(((n * (2 * np.pi / L)) ** 2).sum(axis=1)))
        return tab[:, dim + 1], tab[:, dim + 2]
    if base == "nk_vpi":
        _, qsh, mult = E["nk_shells"]
        tab = _table(path, (qsh.size, 4))
        assert close(tab[:, 0], qsh) and np.array_equal(tab[:, 3], mult)
        return tab[:, 1], tab[:, 2]
    if base == "nrvec_vpi":
        tab = _table(path, (NK_NBIN ** dim, dim + 2))
        j = np.arange(NK_NBIN ** dim)
        for k in range(dim):
            x = -0.5 * L[k] + ((j // NK_NBIN ** k) % NK_NBIN + 0.5) * (L[k] / NK_NBIN)
            assert np.allclose(tab[:, k], x, rtol=PRINT, atol=PRINT * L[k])
        return tab[:, dim], tab[:, dim + 1]
    assert base == "tau_vpi"
    rows = _rows(path)
    M = 2 * Nb + 1
    assert [len(r) for r in rows] == [10] * (M - 1) + [8]
    assert [r[0] for r in rows] == list(range(M)) and close([r[1] for r in rows], (np.arange(M) - Nb) * dt)
    tab = np.array([r + [0.0, 0.0] * (10 - len(r) > 0) for r in rows])  # slice 2Nb starts no link: expectation 0, error 0
    return tab[:, 2::2], tab[:, 3::2]


def check_file(d, base, w, rep, E, what):
    """One file against the expectation: walker w's file, or the walker-averaged one with w = None."""
    bv, bb = E[base]
    cnt = E["counted_of"].get(base, E["counted"])                      # (momentum's files: the blocks that normalise n(k))
    several = rep["W"] > 1
    suffix = f".w{w:04d}" if (w is not None and several) else ""
    got = read_file(d, base, suffix, rep, E)
    mean, err = np.asarray(got[0], np.float64), np.asarray(got[1], np.float64)
    wm, we, n = bs.walker_stats(bv, cnt, w) if w is not None else bs.average_stats(bv, cnt)
    mb = bs.mean_bound(bb, cnt, w) if bb is not None else np.zeros(wm.shape)
    if base == "msd_vpi":                                              # the file's mean and error are those of <dr^2>
        wm, we, mb = wm[:, :1], we[:, :1], mb[:, :1]
    wm, we, mb = wm.reshape(mean.shape), we.reshape(err.shape), mb.reshape(mean.shape)
    tag = f"{what} {base}{suffix}.out"
    if n == 0:                                                         # never diagonal: the reference writes NaN columns too
        assert np.all(np.isnan(mean)) and np.all(np.isnan(err)), tag
        return
    mtol = PRINT * np.abs(wm) + mb
    dm = np.abs(mean - wm)
    worst = float(np.max(np.where(dm == 0, 0.0, dm / np.maximum(mtol, 1e-300))))
    assert np.all(np.isfinite(mean)) and np.all(dm <= mtol), (tag, "means: worst err / bound", worst)
    etol = np.sqrt(4.0 * np.abs(wm) * mtol) + PRINT * np.abs(we)
    ill = we <= etol                                                   # from the expectation alone
    nan = np.isnan(err)
    # (a row of fqt_vpi and tau_vpi carries several estimates, the last axis; elsewhere every element is a row)
    rows = nan.any(axis=-1).ravel() if base in ("fqt_vpi", "tau_vpi", "bo_vpi") else nan.any(axis=0) if base == "boh_vpi" else nan.ravel()
    assert not np.any(nan & ~ill), (tag, "NaN error bars where the expectation is well-conditioned")
    assert rows.sum() <= 0.01 * rows.size, (tag, "rows left out", int(rows.sum()), rows.size)
    de = np.where(nan, 0.0, np.abs(err - we))
    worst_e = float(np.max(np.where(de == 0, 0.0, de / np.maximum(etol, 1e-300))))
    print(f"{tag}: n = {n}, means worst err / bound {worst:.3e}, errors {worst_e:.3e}, NaN rows {int(rows.sum())} of {rows.size}")
    assert np.all(err[~nan] >= 0) and np.all(de <= etol), (tag, "errors: worst err / bound", worst_e)
    if n > 1:
        assert np.any(we > etol), (tag, "no well-conditioned error bar in the file: the check has no teeth")
    if base == "v3tau_vpi":                                            # the mean number of triplets: counts over samples
        m, _, _ = (bs.walker_stats(E["v3_ntrip"], cnt, w) if w is not None else bs.average_stats(E["v3_ntrip"], cnt))
        assert np.all(np.abs(got[2] - m) <= PRINT * np.abs(m)) and m.any(), tag
    if base == "msd_vpi":
        m, _, _ = (bs.walker_stats(bv, cnt, w) if w is not None else bs.average_stats(bv, cnt))
        dim = rep["cfg"].dim
        assert got[2][0] == 0.0 and mean[0, 0] == 0.0                  # lag 0
        a2 = dim * m[1:, 1] / ((dim + 2.0) * m[1:, 0] ** 2) - 1.0
        assert np.all(np.abs(got[2][1:] - a2) <= (3e-12 + 2 * PRINT) * (np.abs(a2) + 1.0)), tag


def check_pressure(d, w, rep, E, what):
    """press_vpi.out: one row per counted block: block, W/Np over the window, Kin/Np as e_vpi.out prints it, and
    P = density/dim (2 Kin/Np - W/Np); tolerance of test_gpu_tau.py / test_gpu_ortho_box.py."""
    cfg = rep["cfg"]
    Nb, dim, dens = cfg.Nb, cfg.dim, cfg.density
    suffix = f".w{w:04d}" if w is not None else ""
    Tq, Tb = E["tau_vpi"]
    cnt = E["counted"]
    if w is None:
        (Tq, cb), Tb = bs.walker_average(Tq, cnt), bs.walker_average(Tb, cnt)[0]
    else:
        Tq, Tb, cb = Tq[w], Tb[w], cnt[w]
    pr = np.array(_rows(os.path.join(d, f"press_vpi{suffix}.out"))).reshape(-1, 4)
    ev = np.array(_rows(os.path.join(d, f"e_vpi{suffix}.out"))).reshape(-1, 4)
    blocks = (np.flatnonzero(cb) + 1).tolist()
    assert pr[:, 0].tolist() == blocks and ev[:, 0].tolist() == blocks, (what, suffix)
    assert open(os.path.join(d, f"press_vpi{suffix}.out")).readline().startswith(f"# block, W/Np = <sum r dv/dr>/Np over the slices Nb-{WINDOW}..Nb+{WINDOW}")
    for row, e, k in zip(pr, ev, np.flatnonzero(cb)):
        wwin = Tq[k, Nb - WINDOW:Nb + WINDOW + 1, 2].mean()
        wb = Tb[k, Nb - WINDOW:Nb + WINDOW + 1, 2].mean()
        assert row[2] == e[2], (what, suffix, k)                       # Kin/N as e_vpi.out has it
        assert abs(row[1] - wwin) <= wb + PRINT * abs(wwin), (what, suffix, k, row[1], wwin)
        want = bs.pressure(row[2], wwin, dens, dim)
        tolp = dens / dim * wb + 5.0000001e-10 * (abs(row[3]) + dens / dim * (2 * abs(row[2]) + abs(wwin)))
        assert abs(row[3] - want) <= tolp, (what, suffix, k, row[3], want)


def _block_rows(d, name, w, cnt, what):
    """The rows of a file with one line per block, whose block numbers are those of the counted blocks: walker w's, or with
    w = None those that some walker counted.  Returns (rows, indices of the blocks)."""
    cb = cnt[w] if w is not None else cnt.any(axis=0)
    rows = np.array(_rows(os.path.join(d, name + (f".w{w:04d}" if w is not None else "") + ".out"))).reshape(-1, 3)
    assert rows[:, 0].tolist() == (np.flatnonzero(cb) + 1).tolist(), (what, name, w, rows[:, 0].tolist(), cb.tolist())
    return rows, np.flatnonzero(cb)


def check_v3(d, w, rep, E, what):
    """v3_vpi.out: one row per counted block: block, V3/Np over the window and P3 = 9 density (V3/Np) / dim."""
    cfg, cnt = rep["cfg"], E["counted"]
    v, vb = E["v3_vpi"]
    if w is None:
        v, vb = bs.walker_average(v, cnt)[0], bs.walker_average(vb, cnt)[0]
    else:
        v, vb = v[w], vb[w]
    rows, blocks = _block_rows(d, "v3_vpi", w, cnt, what)
    k = 9.0 * cfg.density / cfg.dim
    assert np.all(np.abs(rows[:, 1] - v[blocks]) <= vb[blocks] + PRINT * np.abs(v[blocks])), (what, w, rows[:, 1], v[blocks])
    assert np.all(np.abs(rows[:, 2] - k * v[blocks]) <= k * vb[blocks] + PRINT * k * np.abs(v[blocks])), (what, w)
    assert np.all(np.abs(rows[:, 2] - k * rows[:, 1]) <= 2 * PRINT * np.abs(rows[:, 2])) and v[blocks].all(), (what, w)


def check_n0(d, w, rep, E, what):
    """n0_vpi.out: one row per block that normalises n(k): block, n0 = n(0) / Np, n(0) -- counts over CWorm zconf Nobdm."""
    cnt, n0 = E["counted_of"]["n0_vpi"], E["n0"]
    rows, blocks = _block_rows(d, "n0_vpi", w, cnt, what)
    want = (n0[w] if w is not None else bs.walker_average(n0, cnt)[0])[blocks]
    assert np.all(np.abs(rows[:, 1] - want) <= PRINT * want), (what, w, rows[:, 1], want)
    assert np.all(np.abs(rows[:, 2] - want * rep["cfg"].Np) <= PRINT * want * rep["cfg"].Np), (what, w)


def check_replay_is_the_run(d, out, rep):
    """The replay is valid only if it is the run: the final worldlines bit for bit, the diagonal blocks of every walker
    (the rows of its e_vpi file) and the diagonal steps of every block (the run's own figure, printed with two decimals)."""
    cfg, W = rep["cfg"], rep["W"]
    P = np.fromfile(os.path.join(d, "worldlines_final.bin")).reshape((W,) + tuple(cfg.path_shape))
    for w in range(W):
        assert same_bits(P[w], rep["final"][w]), f"replay bug: walker {w}'s final worldline is not the run's"
    S = _blocks(rep["diag"].astype(np.int64), rep)
    for w in range(W):
        rows = _rows(os.path.join(d, f"e_vpi.w{w:04d}.out" if W > 1 else "e_vpi.out"))
        assert [int(r[0]) for r in rows] == (np.flatnonzero(S[w] > 0) + 1).tolist(), f"replay bug: walker {w}'s diagonal blocks"
    pct = [float(ln.split("=")[1].split("%")[0]) for ln in out.splitlines() if "Diagonal conf." in ln]
    assert len(pct) == rep["Nblock"]
    assert np.all(np.abs(np.array(pct) - 100.0 * S.sum(axis=0) / (rep["Nstep"] * W)) <= 0.00501), "replay bug: diagonal steps per block"


def check_run(d, out, rep, E, keys, what, per_walker=True):
    check_replay_is_the_run(d, out, rep)
    for key in keys:
        for base in [f for f in FILES[key] if f in E]:
            if per_walker:
                for w in range(rep["W"]):
                    check_file(d, base, w, rep, E, what)
            check_file(d, base, None, rep, E, what)
    for w in (list(range(rep["W"])) if per_walker else []) + [None]:
        if "tau_profile" in keys and not rep["cfg"].trap:
            check_pressure(d, w, rep, E, what)
        if "three_body" in keys:
            check_v3(d, w, rep, E, what)
        if "momentum" in keys:
            check_n0(d, w, rep, E, what)


def _same(a, b, f):
    return open(os.path.join(a, f), "rb").read() == open(os.path.join(b, f), "rb").read()


# ---- A: a diagonal periodic run, every periodic key in one run ---------------------------------------------------------
A_KEYS = ["fq_tau", "sq_vector", "fq_vector", "fq_self", "gr_vector", "tau_profile"]
NEW_DIAGONAL = ["bond_order", "van_hove", "triplet", "three_body"]
A_PLUS = A_KEYS + NEW_DIAGONAL


@pytest.fixture(scope="module")
def scn_a(gpu_lib, oracle):
    txt, cfg = _input("he4_bis_cworm0_s1982", 3, 4)
    rep = replay(gpu_lib, oracle, cfg, 3, 3, 4)
    assert rep["diag"].all()
    return txt, rep, expectation(rep, A_PLUS)


@gpu
@pytest.mark.parametrize("ds", ["T", "F"])
def test_diagonal_run_every_key_three_blocks(exe, scn_a, tmp_path, ds):
    """he4_bis_cworm0_s1982, Nblock = 3, Nstep = 4, three walkers, the six periodic keys in one run: every file, per
    walker and walker-averaged, means and errors, index columns, and press_vpi.out per block.  With the device sampler a
    second and third run with one key each (the first and the last estimator of the all-reduced vector): the key's files
    are the same characters as in the run with every key on."""
    txt, rep, E = scn_a
    d = str(tmp_path / "all")
    out = _run(exe, txt + _gpu_group(A_KEYS, 3, f"device_sampler = {ds}, "), d)
    check_run(d, out, rep, E, A_KEYS, f"A ds {ds}:")
    if ds == "T":
        for key in ("sq_vector", "fq_self", "tau_profile"):
            one = str(tmp_path / key)
            _run(exe, txt + _gpu_group([key], 3, f"device_sampler = {ds}, "), one)
            for base in FILES[key] + (["press_vpi"] if key == "tau_profile" else []):
                for suffix in [""] + [f".w{w:04d}" for w in range(3)]:
                    assert _same(d, one, f"{base}{suffix}.out"), (key, base, suffix)


@gpu
def test_profiles_normalisations_equal_the_helper(scn_a):
    """pathintegralgroundstate_amd.profiles on the same raw block sums gives the helper's block values: the Python
    post-processing, the Fortran (through the files above) and the helper are three statements of one normalisation."""
    from pathintegralgroundstate_amd import profiles as pf
    import sqv_numpy
    _, rep, E = scn_a
    cfg, raw, S = rep["cfg"], E["raw"], E["samples"]
    Np, dim, L = cfg.Np, cfg.dim, cfg.Lbox
    eq = lambda a, b: np.allclose(a, b, rtol=1e-13, atol=0)
    assert eq(pf.normalize_fqt({"F": raw["fqt"], "samples": S}, Np, WINDOW, cfg.dt, L)[0], E["fqt_vpi"][0])
    assert eq(pf.normalize_sqv(raw["sqv"], S, Np, WINDOW), E["sqvec_vpi"][0])
    assert eq(pf.normalize_fqv(raw["fqv"], S, Np, WINDOW), E["fqvec_vpi"][0])
    assert eq(pf.normalize_fqs(raw["fqs"], S, Np, WINDOW), E["fqself_vpi"][0])
    msd, a2 = pf.normalize_msd(raw["msd"], S, Np, WINDOW, dim)
    m = E["msd_vpi"][0]
    assert eq(msd, m[..., 0]) and eq(a2[..., 1:], dim * m[..., 1:, 1] / ((dim + 2.0) * m[..., 1:, 0] ** 2) - 1.0)
    g = pf.normalize_grv({"vec": raw["grv"], "radial": raw["grw"], "samples": S}, Np, WINDOW, cfg.density, L, cfg.rbin, dim)
    assert eq(g["g_vec"].reshape(E["grvec_vpi"][0].shape), E["grvec_vpi"][0]) and eq(g["g_r"], E["grw_vpi"][0])
    t = pf.normalize_tau({"Q": raw["tau"], "samples": S}, Np, dim, cfg.dt)
    T = E["tau_vpi"][0]
    assert eq(t["vpair"], T[..., 0]) and eq(t["w"], T[..., 2]) and eq(t["klink"], T[..., :-1, 3]) and not T[..., 1].any()
    assert eq(pf.pressure_virial(1.25, t["w"][0, 0, cfg.Nb], cfg.density, dim), bs.pressure(1.25, T[0, 0, cfg.Nb, 2], cfg.density, dim))
    n = sqv_numpy.vectors(dim, NMAX)
    q, mean, mult = pf.shell_average(n, L, E["fqvec_vpi"][0])
    assert eq(q, E["shells"][1]) and np.array_equal(mult, E["shells"][2]) and eq(mean, E["fqsh_vpi"][0])
    assert eq(pf.shell_average(n, L, E["sqvec_vpi"][0])[1], E["sq_vpi"][0])
    # the five newer families
    gd = E["grid"]
    b = pf.normalize_bop({"S": raw["boS"], "H": raw["boH"], "G": raw["boG"], "GN": raw["boGN"], "samples": S}, Np, WINDOW)
    assert eq(np.stack([b[k] for k in ("Q4", "Q6", "q4", "q6", "coordination")], axis=-1), E["bo_vpi"][0])
    assert eq(np.stack([b["P4"], b["P6"]], axis=-2), E["boh_vpi"][0]) and eq(np.nan_to_num(b["G6"], nan=0.0), E["g6_vpi"][0])
    assert np.array_equal(np.isnan(b["G6"]), raw["boGN"] == 0) and E["g6_vpi"][0].any()
    v = pf.normalize_vh({"self": raw["vhs"], "distinct": raw["vhd"], "samples": S}, Np, WINDOW, cfg.density, cfg.rbin, gd["vh_sbin"], dim)
    assert eq(v["G_s"], E["gs_vpi"][0]) and eq(v["G_d"], E["gd_vpi"][0]) and E["gd_vpi"][0].any()
    g = pf.normalize_g3({"trip": raw["g3t"], "pair": raw["g3p"], "samples": S}, Np, WINDOW, cfg.density, gd["g3_rbin"], dim)
    assert eq(g["g3"], E["g3_vpi"][0]) and eq(pf.bond_angle(raw["g3t"], gd["g3_nr"]), E["g3ang_vpi"][0]) and E["g3ang_vpi"][0].any()
    a = pf.normalize_atm({"T": raw["atm"], "ntrip": raw["atm_n"], "samples": S}, Np, nu=gd["atm_nu"])
    assert eq(a["v3"], E["v3tau_vpi"][0]) and eq(a["v3_mean"], E["v3_vpi"][0]) and eq(a["ntrip"], E["v3_ntrip"])
    _, _, win, p3 = bs.norm_atm(raw["atm"], raw["atm_n"], S, Np, gd["atm_nu"], cfg.density, dim)
    assert eq(pf.pressure_atm(a["v3_mean"], cfg.density, dim), p3) and p3.all()


@gpu
def test_profiles_momentum_normalisations_equal_the_helper(scn_b):
    """profiles.normalize_nk and normalize_nrvec on the sums of the blocks that normalise n(k), with their zconf."""
    from pathintegralgroundstate_amd import profiles as pf
    _, rep, E = scn_b
    cfg, raw = rep["cfg"], E["raw"]
    norm = E["counted_of"]["nkvec_vpi"]
    eq = lambda a, b: np.allclose(a[norm], b[norm], rtol=1e-13, atol=0)
    z = np.where(norm, E["zconf"], 1)
    k = pf.normalize_nk({"C": raw["nkC"], "nopen": raw["nkno"]}, cfg.CWorm, z, cfg.Nobdm, cfg.Np, n=rep["nk"]["n"], Lbox=cfg.Lbox)
    vec = E["nkvec_vpi"][0]
    assert eq(k["nk"], vec[..., 1:]) and eq(k["nk0"], vec[..., 0]) and eq(k["n0"], E["n0"]) and eq(k["nk_shell"], E["nk_vpi"][0])
    assert np.allclose(k["k"], E["nk_shells"][1], rtol=1e-13, atol=0) and np.array_equal(k["mult"], E["nk_shells"][2])
    H = raw["nkH"].reshape(raw["nkH"].shape[:2] + (NK_NBIN,) * cfg.dim)
    r = pf.normalize_nrvec({"H": H}, cfg.CWorm, z, cfg.Nobdm, cfg.density, cfg.Lbox, cfg.dim)["rho1"]
    assert eq(r.reshape(E["nrvec_vpi"][0].shape), E["nrvec_vpi"][0]) and vec[norm].any() and E["nrvec_vpi"][0][norm].any()


# ---- B, D: a worm run: samples differ from Nstep, blocks without a sample ----------------------------------------------
B_KEYS = ["sq_vector", "fq_vector", "fq_self", "gr_vector", "tau_profile"]
B_PLUS = B_KEYS + NEW_DIAGONAL + ["momentum"]


@pytest.fixture(scope="module")
def scn_b(gpu_lib, oracle):
    txt, cfg = _input("he4_wormbusy_s7", B_BLOCKS, B_STEPS)
    assert cfg.CWorm > 0
    rep = replay(gpu_lib, oracle, cfg, B_WALKERS, B_BLOCKS, B_STEPS, nk=(NK_NMAX, NK_NBIN))
    S = _blocks(rep["diag"].astype(np.int64), rep)
    print("scenario B: diagonal steps per (walker, block):", S.tolist())
    # what the scenario is for, asserted on the replay before any file is looked at
    assert (S == 0).any(), "no (walker, block) without a diagonal sample"
    assert ((S >= 1) & (S <= B_STEPS - 1)).any(), "no (walker, block) with 1 .. Nstep - 1 samples"
    # momentum counts its blocks by a rule of its own: the sampler's event log and the open flags agree on the diagonal steps,
    # and blocks exist that the diagonal families count and n(k) does not normalise, and the reverse
    assert np.array_equal(rep["zdiag"], rep["diag"])
    norm, zconf, first = momentum_blocks(S, B_STEPS)
    print("scenario B: blocks that normalise n(k):", norm.astype(int).tolist(), "zconf:", zconf.tolist())
    assert ((S > 0) & ~norm).any() and (norm & (first < np.arange(B_BLOCKS))).any(), "momentum's rule does not show"
    assert (zconf[norm] > B_STEPS).any() and rep["nk"]["nopen"].sum() > 0
    return txt, rep, expectation(rep, B_PLUS)


@gpu
def test_worm_run_partial_and_empty_blocks(exe, scn_b, tmp_path):
    """he4_wormbusy_s7 (walker 1 is he4_wormbusy_s8's chain), device sampler, five keys: the sample count of a block is
    the number of its diagonal steps, not Nstep; a block without one is skipped, not counted, and leaves nothing behind
    for the walker's next block.  One key again with the host-driven sampler: the same characters."""
    txt, rep, E = scn_b
    d = str(tmp_path / "T")
    out = _run(exe, txt + _gpu_group(B_KEYS, B_WALKERS, "device_sampler = T, "), d)
    check_run(d, out, rep, E, B_KEYS, "B ds T:")
    h = str(tmp_path / "F")
    out = _run(exe, txt + _gpu_group(["fq_vector"], B_WALKERS, "device_sampler = F, "), h)
    check_run(h, out, rep, E, ["fq_vector"], "B ds F:")
    for base in FILES["fq_vector"]:
        for suffix in [""] + [f".w{w:04d}" for w in range(B_WALKERS)]:
            assert _same(d, h, f"{base}{suffix}.out"), (base, suffix)


@gpu
def test_worm_run_sharded_against_the_replay(exe, scn_b, tmp_path):
    """Scenario B on two contexts of one GPU (n_gpus = 2, same_device = T): the walker-averaged files, whose block values
    meet in the all-reduced vector, against the replay's expectation -- not only against the unsharded run -- and the
    per-walker files as well."""
    txt, rep, E = scn_b
    d = str(tmp_path)
    out = _run(exe, txt + _gpu_group(B_KEYS, B_WALKERS, "device_sampler = T, device = 0, n_gpus = 2, same_device = T, "), d)
    check_run(d, out, rep, E, B_KEYS, "D sharded:")


# ---- A+, B+, D+: the five newer families where they meet the others --------------------------------------------------
def _suffixes(W):
    return [""] + [f".w{w:04d}" for w in range(W)]


def _same_files(a, b, keys, W):
    for key in keys:
        for base in FILES[key] + BLOCK_FILES.get(key, []):
            for suffix in _suffixes(W):
                assert _same(a, b, f"{base}{suffix}.out"), (key, base, suffix)


@gpu
@pytest.mark.parametrize("ds", ["T", "F"])
def test_diagonal_run_all_ten_keys(exe, scn_a, tmp_path, ds):
    """Scenario A with bond_order, van_hove, triplet and three_body behind the six older keys: a 3D run of the four, all
    ten claims on the block vector in one run, every file per walker and walker-averaged against numpy.  With the device
    sampler: the older keys' files are the same characters as in a run without the four (families behind them on the
    vector do not move them), and bond_order and three_body, the first and the last of the new claims, each alone give the
    same characters as in the run with all ten."""
    txt, rep, E = scn_a
    cfg = rep["cfg"]
    d = str(tmp_path / "all")
    out = _run(exe, txt + _gpu_group(A_PLUS, 3, f"device_sampler = {ds}, ", cfg), d)
    check_run(d, out, rep, E, A_PLUS, f"A+ ds {ds}:")
    if ds == "T":
        for name, keys in (("old", A_KEYS), ("bond_order", ["bond_order"]), ("three_body", ["three_body"])):
            one = str(tmp_path / name)
            _run(exe, txt + _gpu_group(keys, 3, f"device_sampler = {ds}, ", cfg), one)
            _same_files(d, one, keys, 3)


B_HOST = ["van_hove", "momentum"]


@gpu
def test_worm_run_all_families_partial_and_empty_blocks(exe, scn_b, tmp_path):
    """Scenario B with the four diagonal families and momentum behind the five older keys.  The diagonal families: the
    samples of a block are its diagonal steps, a block without one is skipped and leaves nothing behind.  momentum: a block
    normalises n(k) once the walker has Nstep diagonal configurations since its last normalised block, with the sums
    carried over until then, and n0_vpi*.out has exactly those blocks.  van_hove and momentum again with the host-driven
    sampler (pigs_nk_add in place of pigs_nk_accumulate): the same characters."""
    txt, rep, E = scn_b
    cfg = rep["cfg"]
    d = str(tmp_path / "T")
    out = _run(exe, txt + _gpu_group(B_PLUS, B_WALKERS, "device_sampler = T, ", cfg), d)
    check_run(d, out, rep, E, B_PLUS, "B+ ds T:")
    h = str(tmp_path / "F")
    out = _run(exe, txt + _gpu_group(B_HOST, B_WALKERS, "device_sampler = F, ", cfg), h)
    check_run(h, out, rep, E, B_HOST, "B+ ds F:")
    _same_files(d, h, B_HOST, B_WALKERS)


@gpu
def test_worm_run_all_families_sharded_against_the_replay(exe, scn_b, tmp_path):
    """Scenario B with all ten keys on two contexts of one GPU: momentum's block counts and the diagonal families' differ
    per shard and meet in one all-reduced vector; every file against the replay's expectation."""
    txt, rep, E = scn_b
    d = str(tmp_path)
    out = _run(exe, txt + _gpu_group(B_PLUS, B_WALKERS, "device_sampler = T, device = 0, n_gpus = 2, same_device = T, ", rep["cfg"]), d)
    check_run(d, out, rep, E, B_PLUS, "D+ sharded:")


# ---- E: boxes with unequal sides, the defaults that depend on the box left out --------------------------------------
E_KEYS = (f"bond_order = T, bo_rnb = RNB, bo_nhist = {BO_NH}, bo_window = {WINDOW}, van_hove = T, vh_ntau = {NTAU}, "
          f"vh_window = {WINDOW}, vh_nself = {VH_NS}, triplet = T, g3_nr = {G3_NR}, g3_na = {G3_NA}, g3_window = {WINDOW}, "
          f"three_body = T, atm_window = {WINDOW}, atm_nu = {ATM_NU!r}d0")


@gpu
@pytest.mark.parametrize("name,extra", [("ortho2d_sta_s1982", []), ("ortho_worm_s7", ["momentum"])])
def test_unequal_sides_defaults_left_out(gpu_lib, oracle, exe, tmp_path, name, extra):
    """ortho2d_sta_s1982 (2D, sides 5 x 8) and ortho_worm_s7 (3D, worm, sides 3.2 x 4.8 x 6.4), two walkers, Nblock = 2,
    Nstep = 3, with g3_rmax, atm_rc, vh_rself and bo_nr NOT given: half the shortest side, rcut and the run's g(r) grid.
    The namelists cannot state sides that differ, so the run's box (driver.npz: Lbox, density) reaches the front end the
    way he4_crystal_ortho's does, through config_ini.in with crystal = T; every walker starts on its positions (drawn
    here in the box), which the replay starts on as well."""
    from pathintegralgroundstate_amd import SystemConfig
    W, Nblock, Nstep = 2, 2, 3
    txt, _ = _input(name, Nblock, Nstep)
    box = np.load(os.path.join(RUNS, name, "driver.npz"))
    L, dens = [float(x) for x in box["Lbox"]], float(box["density"])
    txt, k = re.subn(r"trap = F", "crystal = T, trap = F", txt)
    Np = int(re.search(r"Np\s*=\s*(\d+)", txt).group(1))
    assert k == 1 and len(set(L)) == len(L) and abs(Np / np.prod(L) / dens - 1) < 1e-14
    cfg = SystemConfig.from_namelists(txt, Np=Np, density=dens, Lbox=L)
    half = 0.5 * min(L)
    assert cfg.rcut == half and max(L) > 1.5 * min(L)
    X = np.random.default_rng(len(L)).uniform(-0.5, 0.5, (Np, cfg.dim)) * np.asarray(L)
    d = str(tmp_path)
    with open(os.path.join(d, "config_ini.in"), "w") as f:
        f.write(f"{Np}\n" + " ".join(repr(x) for x in L) + f"\n{dens!r}\n" + "".join(" ".join(repr(float(x)) for x in r) + "\n" for r in X))
    keys = NEW_DIAGONAL + extra
    rep = replay(gpu_lib, oracle, cfg, W, Nblock, Nstep, nk=(NK_NMAX, NK_NBIN) if extra else None, start=X)
    E = expectation(rep, keys, bo_nr=cfg.Nbin, vh_rself=cfg.rcut)
    gd = E["grid"]
    assert gd["g3_rmax"] == gd["atm_rc"] == gd["vh_rself"] == half and gd["bo_rbin"] == cfg.rbin and gd["rnb"] <= half
    group = f"&gpu\n n_walkers = {W}, device_sampler = T, " + E_KEYS.replace("RNB", f"{gd['rnb']:.6f}d0") + "".join(", " + KEYS[e] for e in extra) + "\n/\n"
    for left_out in ("g3_rmax", "atm_rc", "vh_rself", "bo_nr"):
        assert left_out not in group
    out = _run(exe, txt + group, d)
    # the banner names the values that the run took
    legs = re.search(r"Triplet g3\s*: on \(legs below\s*([0-9.Ee+-]+),", out)
    sides = re.search(r"Three-body V3\s*: on \(nu =\s*[0-9.Ee+-]+, sides below\s*([0-9.Ee+-]+),", out)
    assert legs and sides and float(legs.group(1)) == half and float(sides.group(1)) == half, out[:3000]
    # (momentum is on in the worm run, behind the four on the block vector, and n0_vpi*.out is checked; with three steps per
    # block its block values have no spread, so its three statistics files would be checked without teeth: B+ and D+ have them)
    check_run(d, out, rep, E, NEW_DIAGONAL, f"E {name}:")
    for w in ([0, 1, None] if extra else []):
        check_n0(d, w, rep, E, f"E {name}:")


# ---- C: a trapped run --------------------------------------------------------------------------------------------------
C_KEYS = ["density_profile", "tau_profile"]


@gpu
def test_trapped_run_profiles_three_blocks(gpu_lib, oracle, exe, tmp_path):
    """trap2d_bis_cworm0, two walkers, Nblock = 3, Nstep = 3: dens_vpi, rho_vpi, pr_vpi and tau_vpi, per walker and
    averaged, means and errors."""
    txt, cfg = _input("trap2d_bis_cworm0", 3, 3)
    rep = replay(gpu_lib, oracle, cfg, 2, 3, 3)
    assert cfg.trap and rep["diag"].all()
    E = expectation(rep, C_KEYS)
    d = str(tmp_path)
    out = _run(exe, txt + _gpu_group(C_KEYS, 2, "device_sampler = T, "), d)
    check_run(d, out, rep, E, C_KEYS, "C:")
    assert not os.path.exists(os.path.join(d, "press_vpi.out"))


# ---- L: the lattice family beside the ten periodic diagonal keys, on a crystal -----------------------------------------
L_WALKERS, L_BLOCKS, L_STEPS = 3, 3, 4
L_KEYS = A_PLUS + ["lattice"]
LIND = ("u2_mean", "gamma", "alpha2", "vacant", "multiple", "hops_link", "hops_window")
# mom lies within 1e-12 of itself (test_gpu_lat.py): <u^2> and gamma carry that, alpha_2 + 1 = dim <u^4> / ((dim + 2) <u^2>^2)
# three times that; the other four columns are ratios of integers
LIND_REL = np.array([1e-12, 1e-12, 3e-12, 0.0, 0.0, 0.0, 0.0])


def _crystal_dir(base, name):
    import shutil
    d = os.path.join(str(base), name)
    os.makedirs(d)
    shutil.copy(os.path.join(RUNS, "he4_crystal", "config_ini.in"), d)
    return d


@pytest.fixture(scope="module")
def scn_l(gpu_lib, oracle):
    """he4_crystal: 27 particles started on the sites of config_ini.in, worm sector on.  The raw lattice sums of every
    diagonal step from lat_numpy on the replay's snapshots, the columns from block_stats_numpy.norm_lat."""
    import lat_numpy
    from pathintegralgroundstate_amd import SystemConfig
    W = L_WALKERS
    txt, _ = _input("he4_crystal", L_BLOCKS, L_STEPS)
    ini = open(os.path.join(RUNS, "he4_crystal", "config_ini.in")).read().split("\n")
    Np, L, dens = int(ini[0]), [float(x) for x in ini[1].split()], float(ini[2])
    cfg = SystemConfig.from_namelists(txt, Np=Np, density=dens, Lbox=L)
    assert cfg.CWorm > 0 and cfg.dim == 3
    R = np.array([[float(x) for x in l.split()] for l in ini[3:3 + Np]])
    assert R.shape == (Np, cfg.dim)
    # the sites' nearest-neighbour distance, every difference folded by the nearest multiple of the side
    d = R[:, None, :] - R[None, :, :]
    d = d - np.asarray(L) * np.rint(d / np.asarray(L))
    r2 = (d * d).sum(axis=-1)
    r2[np.diag_indices(Np)] = np.inf
    ann = float(np.sqrt(r2.min()))
    rmax = float(np.floor(0.5 * ann * 1e6) / 1e6)      # six decimals: the namelist and numpy read the same double
    rep = replay(gpu_lib, oracle, cfg, W, L_BLOCKS, L_STEPS, start=R)
    S = _blocks(rep["diag"].astype(np.int64), rep)
    print("scenario L: diagonal steps per (walker, block):", S.tolist())
    steps = []
    for t in range(rep["snaps"].shape[0]):
        ws = [int(w) for w in np.flatnonzero(rep["diag"][t])]
        steps.append(lat_numpy.Window(rep["snaps"][t], cfg.Nb, WINDOW, cfg.Lbox, R, LAT_NBIN, rmax, 1).expected(ws))
    raw = {k: _blocks(np.stack([e[k] for e in steps]), rep) for k in steps[0]}
    cnt = S > 0
    assert np.array_equal(raw["samples"], S) and cnt.any()
    assert (S == 0).any() and ((S >= 1) & (S < L_STEPS)).any(), "no empty or no partial (walker, block)"
    assert (cnt.sum(axis=0) == 1).any() and cnt.any(axis=0).all()       # a block of one walker alone; no block of nobody
    v = bs.norm_lat_raw(raw, Np, Np, ann, rmax)

    def clean(x):
        x = np.array(x, np.float64)
        x[~cnt] = 0.0
        return x

    lind = clean(np.stack([v[k] for k in LIND], axis=-1))
    tau = clean(np.concatenate([v["u2"][..., None], v["uk2"], v["gamma_tau"][..., None]], axis=-1))
    pu = v["pu"]                                                        # [W, Nblock, dim, 2 nbin]: -rmax .. rmax
    cols = [v["rho_site"]]
    for k in range(cfg.dim):
        cols += [pu[..., k, LAT_NBIN - 1::-1], pu[..., k, LAT_NBIN:]]    # P(u_k = -r), P(u_k = +r) at r ascending
    us = clean(np.stack(cols, axis=-1))
    scale = np.abs(lind)
    scale[..., 2] += 1.0
    vals = {"lind_vpi": (lind, (PRINT + LIND_REL) * scale), "lindtau_vpi": (tau, (PRINT + 1e-12) * np.abs(tau)),
            "usite_vpi": (us, PRINT * np.abs(us))}
    assert np.all(lind[cnt][:, 0] > 0) and np.all(lind[cnt][:, 1] < 0.5) and us[cnt].any()
    group = _gpu_group(L_KEYS, W, "device_sampler = T, ", cfg).replace("RMAX", f"{rmax:.6f}d0")
    return dict(txt=txt, rep=rep, cfg=cfg, cnt=cnt, vals=vals, rmax=rmax, group=group)


def check_lattice(d, sc, what, per_walker=True):
    """lind_vpi*.out: one line per block that the walker (or, merged, some walker) counted; lindtau_vpi*.out and
    usite_vpi*.out: the means over those blocks.  Merged: per block the mean over the walkers that counted it."""
    rep, cfg, cnt = sc["rep"], sc["cfg"], sc["cnt"]
    W, dim, ns = rep["W"], cfg.dim, 2 * WINDOW + 1
    for w in (list(range(W)) if per_walker else []) + [None]:
        suffix = f".w{w:04d}" if w is not None else ""
        tag = f"{what} walker {w}"
        v, t = sc["vals"]["lind_vpi"]
        if w is None:
            (v, cb), t = bs.walker_average(v, cnt), bs.walker_average(t, cnt)[0]
        else:
            v, t, cb = v[w], t[w], cnt[w]
        path = os.path.join(d, f"lind_vpi{suffix}.out")
        assert open(path).readline().startswith(f"# block, <u^2> over the slices Nb-{WINDOW}..Nb+{WINDOW}, Lindemann ratio"), tag
        rows = np.array(_rows(path)).reshape(-1, 8)
        blocks = np.flatnonzero(cb)
        assert rows[:, 0].tolist() == (blocks + 1.0).tolist(), (tag, rows[:, 0].tolist(), cb.tolist())
        err = np.abs(rows[:, 1:] - v[blocks])
        assert np.all(np.isfinite(rows)) and np.all(err <= t[blocks]), (tag, "lind", (err / np.maximum(t[blocks], 1e-300)).max())
        index = {"lindtau_vpi": (np.arange(ns) - WINDOW) * cfg.dt, "usite_vpi": (np.arange(LAT_NBIN) + 0.5) * sc["rmax"] / LAT_NBIN}
        for base, ncol in (("lindtau_vpi", 2 + dim), ("usite_vpi", 1 + 2 * dim)):
            v, t = sc["vals"][base]
            m, _, n = bs.walker_stats(v, cnt, w) if w is not None else bs.average_stats(v, cnt)
            assert n == blocks.size
            tab = _table(os.path.join(d, f"{base}{suffix}.out"), (index[base].size, 1 + ncol))
            assert np.allclose(tab[:, 0], index[base], rtol=PRINT, atol=1e-300), (tag, base)
            if n == 0:                                                  # never diagonal: a mean over no block
                assert np.all(np.isnan(tab[:, 1:])), (tag, base)
                continue
            err, tol = np.abs(tab[:, 1:] - m), bs.mean_bound(t, cnt, w)
            assert np.all(np.isfinite(tab)) and np.all(err <= tol), (tag, base, (err / np.maximum(tol, 1e-300)).max())
            assert m.any(), (tag, base)


@pytest.fixture(scope="module")
def run_l(exe, scn_l, tmp_path_factory):
    """Scenario L's run with all eleven keys, unsharded."""
    d = _crystal_dir(tmp_path_factory.mktemp("L"), "all")
    return d, _run(exe, scn_l["txt"] + scn_l["group"], d)


@gpu
def test_crystal_run_lattice_beside_ten_keys(exe, scn_l, run_l, tmp_path):
    """he4_crystal, Nblock = 3, Nstep = 4, three walkers, worm sector on, lattice (window 2, 6 bins) behind the ten
    periodic diagonal keys on one all-reduced block vector.  The replay is the run; the three lattice files of every
    walker and the merged ones -- lind_vpi.out with the walker average of every block that some walker counted,
    lindtau_vpi.out and usite_vpi.out with the all-reduced means -- against lat_numpy on the replay's snapshots and
    norm_lat.  A run with the key alone writes the same characters into all of them.
    Diagonal steps per block of this fixture: walker 0: 4 0 0, walker 1: 4 4 4, walker 2: 1 0 1 -- empty blocks behind a
    counted one, a partial block, a block that one walker alone counted; the scenario asserts that both kinds are there."""
    d, out = run_l
    assert "Lattice sites" in out
    check_replay_is_the_run(d, out, scn_l["rep"])
    check_lattice(d, scn_l, "L all keys:")
    one = _crystal_dir(tmp_path, "alone")
    group = _gpu_group(["lattice"], L_WALKERS, "device_sampler = T, ", scn_l["cfg"]).replace("RMAX", f"{scn_l['rmax']:.6f}d0")
    out1 = _run(exe, scn_l["txt"] + group, one)
    check_replay_is_the_run(one, out1, scn_l["rep"])
    _same_files(d, one, ["lattice"], L_WALKERS)


def superfluid_blocks(rep):
    """The block values of the superfluid family from the replay: the raw sums of every diagonal step from sf_numpy on the
    step's snapshot, added over the steps of a block here, and block_stats_numpy.norm_sf.  Returns ({name: [W, Nblock,
    ..]}, counted [W, Nblock])."""
    import sf_numpy
    cfg = rep["cfg"]
    steps = []
    for t in range(rep["snaps"].shape[0]):
        ws = [int(w) for w in np.flatnonzero(rep["diag"][t])]
        steps.append(sf_numpy.Window(rep["snaps"][t], cfg.Nb, WINDOW, cfg.Lbox[:cfg.dim], SF_NTAU).expected(ws))
    raw = {k: _blocks(np.stack([e[k] for e in steps]), rep) for k in steps[0]}
    S = _blocks(rep["diag"].astype(np.int64), rep)
    assert np.array_equal(raw["samples"], S) and raw["C"].shape == raw["D"].shape == S.shape + (SF_NTAU + 1, cfg.dim)
    return bs.norm_sf(raw["C"], raw["D"], S, WINDOW, cfg.Np, cfg.dt), S > 0


def check_superfluid(d, vals, cnt, rep, what, per_walker=True):
    """rhos_vpi*.out and msdu_vpi*.out of the directory d against the block values: walker w's files take the blocks that
    the walker counted; the all-reduced files take, of every block that some walker counted, the mean over the walkers that
    counted it (block_stats_numpy.walker_average, the rule of pigs_block_stats.f90).  test_sf_host.check_files: the means
    to the printed digits, the block errors to 1e-6 of the values' scale."""
    from test_sf_host import check_files
    cfg, W = rep["cfg"], rep["W"]
    for w in (list(range(W)) if per_walker else []) + [None]:
        if w is None:
            avg = {k: bs.walker_average(v, cnt) for k, v in vals.items()}
            mine, cb = {k: a[0] for k, a in avg.items()}, avg["Dcm"][1]
            assert np.array_equal(cb, cnt.any(axis=0))
        else:
            mine, cb = {k: v[w] for k, v in vals.items()}, cnt[w]
        blocks = [{k: v[b] for k, v in mine.items()} for b in np.flatnonzero(cb)]
        assert blocks, (what, w)
        for b in blocks:                                                # counted: every lag beyond 0 is a number
            assert all(np.all(np.isfinite(b[k][1:])) for k in b) and np.all(b["msd"][1:] > 0), (what, w)
        suffix = f".w{w:04d}" if w is not None else ""
        print(f"{what} rhos_vpi{suffix}.out, msdu_vpi{suffix}.out: {len(blocks)} blocks")
        check_files(os.path.join(d, f"rhos_vpi{suffix}.out"), os.path.join(d, f"msdu_vpi{suffix}.out"), blocks, cfg.dim, SF_NTAU, cfg.dt)


@gpu
def test_crystal_run_superfluid_beside_eleven_keys(exe, scn_l, run_l, tmp_path):
    """Scenario L with superfluid (lags 0..3 of window 2: fewer than the window holds) behind the eleven keys, the last
    claim on the all-reduced block vector.  The expectation is independent of pigs_sf_*: sf_numpy on the replay's
    snapshots, norm_sf, and the block statistics restated in block_stats_numpy.  Checked: the two files of every walker
    (a walker's mean is over the blocks in which it was diagonal and no others: walker 0 counts one block of three, walker
    2 two); the all-reduced rhos_vpi.out and msdu_vpi.out; a run with the key alone writes the same characters into all
    four kinds of file; every file of the run without the key is unchanged byte for byte; on two contexts of one GPU the
    all-reduced files meet the same expectation and the per-walker files are the one-shard run's byte for byte."""
    sc = scn_l
    rep, cfg, cnt, W = sc["rep"], sc["cfg"], sc["cnt"], L_WALKERS
    vals, counted = superfluid_blocks(rep)
    assert np.array_equal(counted, cnt) and cnt.all(axis=1).any() and (cnt.sum(axis=1) < L_BLOCKS).any() and cnt.any(axis=1).all()
    assert SF_NTAU < 2 * WINDOW and not cfg.trap and cfg.Nb >= WINDOW
    group = _gpu_group(L_KEYS + ["superfluid"], W, "device_sampler = T, ", cfg).replace("RMAX", f"{sc['rmax']:.6f}d0")
    assert group.replace(", " + KEYS["superfluid"], "") == sc["group"]
    plain, _ = run_l
    d = _crystal_dir(tmp_path, "all")
    out = _run(exe, sc["txt"] + group, d)
    assert "Superfluid fraction" in out and "Lattice sites" in out
    check_replay_is_the_run(d, out, rep)
    check_superfluid(d, vals, cnt, rep, "S all keys:")
    # the other keys' files: unchanged by the key; the new files: the four kinds and nothing else
    old = sorted(os.listdir(plain))
    new = sorted(set(os.listdir(d)) - set(old))
    assert new == sorted(f"{base}{s}.out" for base in FILES["superfluid"] for s in _suffixes(W)), new
    for f in old:
        if f not in ("stdout.txt", "vpi.in"):
            assert _same(plain, d, f), f
    # the key alone
    one = _crystal_dir(tmp_path, "alone")
    out1 = _run(exe, sc["txt"] + _gpu_group(["superfluid"], W, "device_sampler = T, ", cfg), one)
    check_replay_is_the_run(one, out1, rep)
    _same_files(d, one, ["superfluid"], W)
    # two contexts of one GPU
    two = _crystal_dir(tmp_path, "two")
    out2 = _run(exe, sc["txt"] + group.replace("device_sampler = T, ", "device_sampler = T, device = 0, n_gpus = 2, same_device = T, "), two)
    assert re.search(r"GPUs \(walker shards\):\s*2\b", out2), out2[:3000]
    check_replay_is_the_run(two, out2, rep)
    check_superfluid(two, vals, cnt, rep, "S sharded:", per_walker=False)
    for base in FILES["superfluid"]:
        for w in range(W):
            assert _same(d, two, f"{base}.w{w:04d}.out"), (base, w)


@gpu
def test_crystal_run_lattice_sharded(exe, scn_l, run_l, tmp_path):
    """Scenario L on two contexts of one GPU (two walkers and one): the merged files, whose block values meet in the
    all-reduced vector, against the expectation and, number for number to the printed digits, against the unsharded run;
    the per-walker files byte for byte."""
    d, _ = run_l
    two = _crystal_dir(tmp_path, "two")
    out = _run(exe, scn_l["txt"] + scn_l["group"].replace("device_sampler = T, ", "device_sampler = T, device = 0, n_gpus = 2, same_device = T, "), two)
    assert re.search(r"GPUs \(walker shards\):\s*2\b", out), out[:3000]
    check_replay_is_the_run(two, out, scn_l["rep"])
    check_lattice(two, scn_l, "L sharded:")
    for base in FILES["lattice"]:
        for w in range(L_WALKERS):
            assert _same(d, two, f"{base}.w{w:04d}.out"), (base, w)
        a, b = np.array(_rows(os.path.join(d, base + ".out"))), np.array(_rows(os.path.join(two, base + ".out")))
        assert a.shape == b.shape and np.allclose(a, b, rtol=2 * PRINT, atol=2 * PRINT, equal_nan=True), base
