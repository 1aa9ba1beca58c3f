"""Wrapping clusters, the finite clusters' unfolded Rg^2 and cluster persistence on the MI355X (pigs_pc_*, pigs_pc.hip),
through the C ABI.

The expected sums come from the numpy restatement in tests/pc_numpy.py (a union-find with offset vectors, another
algorithm than the device's sweeps; pinned by tests/test_pc_numpy_host.py).  Every integer array must be EQUAL; rg2u lies
within 1e-12 * Sum|terms| per element, the project's bound for a fixed-order sum (the terms are non-negative, so Sum|terms|
is the expected value itself), and has the restatement's bits where an element holds one term.  No comparison masks or
skips elements.

Largest |got - want| / bound seen on the MI355X: see DESIGN.md (the percolation section)."""
import ctypes as C

import numpy as np
import pytest

import cl_numpy as cn
import pc_numpy as pn
from helpers import same_bits
from pathintegralgroundstate_amd import SystemConfig
from test_gpu_cl import ADJ_MAX, CHAIN_L, DENSITY, ST, _cfg, _flat

pytestmark = pytest.mark.gpu
INTS = ("nwrap", "mwrap", "swrap", "nfin", "samples", "first", "second", "both", "norig")
SECOND_RADIUS = 0.8                                                     # of threshold_rc: mostly finite clusters (probed on the CPU)
_ip = C.POINTER(C.c_int32)
HB = pn.hand_built()


def _assert_same(got, exp, what):
    for k in INTS:
        assert got[k].dtype == np.int64 and got[k].shape == exp[k].shape, (what, k)
        assert np.array_equal(got[k], exp[k]), (what, k, got[k], exp[k])
    assert got["rg2u"].shape == exp["rg2u"].shape and got["rg2u"].dtype == np.float64, what
    bound = 1e-12 * np.abs(exp["rg2u"])
    err = np.abs(got["rg2u"] - exp["rg2u"])
    with np.errstate(all="ignore"):
        worst = float(np.max(np.where(err == 0, 0.0, err / bound), initial=0.0))
    print(f"{what}: max |got-want|/bound of rg2u = {worst:.3e} over {err.size} elements")
    assert np.all(err <= bound), (what, worst)
    one = exp["terms"] <= 1
    assert same_bits(got["rg2u"][one], exp["rg2u"][one]), (what, "an element of one term")


def _same(a, b, what=""):
    for k in INTS:
        assert np.array_equal(a[k], b[k]), (what, k)
    assert same_bits(a["rg2u"], b["rg2u"]), (what, "rg2u")


def _run(gpu_lib, cfg, P, rc, window, ntau, lists, also=None):
    VT, WF = gpu_lib.build_tables(cfg)
    with gpu_lib.PigsContext(cfg, VT, WF, n_walkers=P.shape[0]) as ctx:
        ctx.upload_all(P)
        ctx.pc_init(rc, window, ntau)
        for wl in lists:
            ctx.pc_accumulate(wl)
        got = ctx.pc_read()
        return (got, also(ctx)) if also else got


# ---- 1. random configurations in a box of unequal sides -----------------------------------------------------------------
@pytest.mark.parametrize("Np", [2, 3, 64, 65, 257, 300])
@pytest.mark.parametrize("dim", [1, 2, 3])
def test_matches_numpy(gpu_lib, dim, Np):
    """test_gpu_cl.py::test_matches_numpy's inputs and walker lists; windows 0, 2 and Nb on one context (pc_init again
    resizes and zeroes) with ntau = min(2, 2 window); the threshold radius, where nearly every slice wraps, and 0.8 of it."""
    Nb, W = 3, 3
    cfg = _cfg(dim, Np, Nb)
    L = cfg.Lbox[:dim]
    P = cn.random_paths(W, 2 * Nb + 1, Np, L, np.random.default_rng(100 * dim + Np))
    lists = [[2, 1], [0], [1]]
    VT, WF = gpu_lib.build_tables(cfg)
    slice_masks, cluster_masks = set(), set()
    with gpu_lib.PigsContext(cfg, VT, WF, n_walkers=W) as ctx:
        ctx.upload_all(P)
        for factor in (1.0, SECOND_RADIUS):
            rc = factor * cn.threshold_rc(dim, DENSITY[dim], L)
            for window in (0, 2, Nb):
                ntau = min(2, 2 * window)
                exp = pn.Window(P, Nb, window, L, rc, ntau).expected(_flat(lists, W))
                if window == Nb:
                    slice_masks |= set(np.nonzero(exp["swrap"].sum(axis=0))[0].tolist())
                    cluster_masks |= set(np.nonzero(exp["nwrap"].sum(axis=0))[0].tolist())
                ctx.pc_init(rc, window, ntau)
                for wl in lists:
                    ctx.pc_accumulate(wl)
                got = ctx.pc_read()
                assert (got["window"], got["ntau"]) == (window, ntau)
                assert got["samples"].tolist() == [2 * window + 1, 2 * (2 * window + 1), 2 * window + 1]
                _assert_same(got, exp, f"dim {dim} Np {Np} rc x {factor} window {window}")
    if dim >= 2 and Np >= 64:                                           # on the restatement alone
        assert 0 in slice_masks and slice_masks - {0}, "the case lacks wrapping or non-wrapping slices"
        assert len(cluster_masks - {0}) >= 2, "fewer than two distinct non-zero masks"


# ---- 2. hand-built slices at window 0 ---------------------------------------------------------------------------------
def _one_slice(gpu_lib, X, Lbox, rc, cl=False):
    """X as the middle slice of one walker (window 0): (got, expected, (labelling, image) sweeps, cl_read or None)."""
    dim, Np = X.shape[1], X.shape[0]
    cfg = _cfg(dim, Np, 1, Lbox=list(Lbox))
    P = cn.as_paths(X, 3)
    exp = pn.Window(P, 1, 0, Lbox, rc).expected([0])

    def also(ctx):
        sweeps = ctx.pc_sweeps()
        if not cl:
            return sweeps, None
        ctx.cl_init(rc, 0)                                              # beside the initialised pc family
        ctx.cl_accumulate()
        ctx.pc_accumulate()
        again = ctx.pc_read()
        return sweeps, (ctx.cl_read(), again)

    got, (sweeps, other) = _run(gpu_lib, cfg, P, rc, 0, 0, [None], also=also)
    return got, exp, sweeps, other


@pytest.mark.parametrize("name", sorted(HB))
def test_hand_built(gpu_lib, name):
    """Every slice that tests/test_pc_numpy_host.py pins."""
    X, L, rc = HB[name]
    got, exp, sweeps, _ = _one_slice(gpu_lib, X, L, rc)
    _assert_same(got, exp, name)
    Np = X.shape[0]
    print(f"{name}: {sweeps[0]} labelling sweeps, {sweeps[1]} image sweeps")
    assert 1 <= sweeps[1] <= Np and 1 <= sweeps[0] <= Np + 1
    if name.startswith("ring"):
        assert got["nwrap"][0].tolist() == [0, 1, 0, 0, 0, 0, 0, 0] and got["mwrap"][0, 1] == Np and got["swrap"][0, 1] == 1
    if name == "staircase":
        assert got["nwrap"][0, 3] == 1 and got["swrap"][0, 3] == 1
    if name.endswith("d_bonded"):
        assert got["mwrap"][0, (1 << X.shape[1]) - 1] == Np


def test_cut_ring_differs_from_the_folded_rg2(gpu_lib):
    X, L, rc = HB["cut_ring"]
    got, exp, _, (cl, again) = _one_slice(gpu_lib, X, L, rc, cl=True)
    s = X.shape[0]
    _assert_same(got, exp, "cut ring")
    assert cl["nsize"][0, s - 1] == 1 and got["nfin"][0, s - 1] == 1
    assert got["rg2u"][0, s - 1] > 1.5 * cl["rg2"][0, s - 1] > 0
    assert np.array_equal(again["nfin"], 2 * got["nfin"])


def test_short_chain_has_the_bits_of_cl(gpu_lib):
    """A chain shorter than half the box, both families initialised on the one context: rg2u carries cl_read()["rg2"]'s bits."""
    n, rc = 40, 1.0
    X = cn.chain(n, 0.9 * rc, np.random.default_rng(40).permutation(n), origin=[-140.0, 1.0, -2.0])
    got, exp, _, (cl, _) = _one_slice(gpu_lib, X, CHAIN_L, rc, cl=True)
    _assert_same(got, exp, "short chain")
    assert got["nfin"][0, n - 1] == 1 and got["nwrap"][0].tolist() == [1, 0, 0, 0, 0, 0, 0, 0]
    assert got["rg2u"][0, n - 1] > 0 and same_bits(got["rg2u"], cl["rg2"])


# ---- 3. both adjacency forms ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Np", [ADJ_MAX, ADJ_MAX + 1])
def test_both_adjacency_forms(gpu_lib, Np):
    """The bit rows in LDS up to kClAdjNpMax particles, the distances of every sweep beyond: a slice with a wrapping and
    a finite cluster of several particles."""
    assert ADJ_MAX == 256
    cfg = _cfg(3, Np, 1)
    rc = cn.threshold_rc(3, DENSITY[3], cfg.Lbox)
    P = cn.random_paths(1, 3, Np, cfg.Lbox, np.random.default_rng(Np))
    exp = pn.Window(P, 1, 0, cfg.Lbox, rc).expected([0])
    assert exp["nwrap"][0, 1:].sum() >= 1 and exp["nfin"][0, 1:].sum() >= 1 and np.any(exp["rg2u"][0] > 0)
    _assert_same(_run(gpu_lib, cfg, P, rc, 0, 0, [None]), exp, f"form at Np {Np}")


# ---- 4. persistence ---------------------------------------------------------------------------------------------------
def test_identical_slices_keep_every_pair(gpu_lib):
    cfg = _cfg(2, 60, 2)
    L = cfg.Lbox[:2]
    rc = cn.threshold_rc(2, DENSITY[2], L)
    P = cn.as_paths(cn.random_paths(1, 1, 60, L, np.random.default_rng(8))[0, 0], 5)
    got = _run(gpu_lib, cfg, P, rc, 2, 4, [None])
    _assert_same(got, pn.Window(P, 2, 2, L, rc, 4).expected([0]), "identical slices")
    assert got["first"][0, 0] > 0 and np.array_equal(got["both"], got["first"]) and np.array_equal(got["both"], got["second"])
    assert got["norig"][0].tolist() == [5, 4, 3, 2, 1]


def test_alternating_partitions_have_the_known_counts(gpu_lib):
    """Six particles; even slices hold the pairs {0,1} {2,3} {4,5}, odd ones the triples {0,1,2} {3,4,5}: 3 pairs against
    6, of which {0,1} and {4,5} are together in both."""
    L, rc = [12.0, 12.0], 0.5
    A = np.array([[0, 0], [.25, 0], [3, 0], [3.25, 0], [-3, 3], [-3.25, 3]], float)
    B = np.array([[0, 0], [.25, 0], [.5, 0], [-3.5, 3], [-3, 3], [-3.25, 3]], float)
    P = np.stack([A, B, A, B, A])[None]
    cfg = _cfg(2, 6, 2, Lbox=L)
    got = _run(gpu_lib, cfg, P, rc, 2, 4, [None])
    _assert_same(got, pn.Window(P, 2, 2, L, rc, 4).expected([0]), "alternating")
    assert got["norig"][0].tolist() == [5, 4, 3, 2, 1]
    assert got["first"][0].tolist() == [3 * 3 + 6 * 2, 2 * 3 + 2 * 6, 2 * 3 + 6, 3 + 6, 3]
    assert got["second"][0].tolist() == [21, 2 * 6 + 2 * 3, 2 * 3 + 6, 6 + 3, 3]
    assert got["both"][0].tolist() == [21, 4 * 2, 12, 2 * 2, 3]


@pytest.mark.parametrize("Np", [65, 257])
def test_random_paths_over_every_lag(gpu_lib, Np):
    Nb, W, window = 3, 2, 3
    cfg = _cfg(3, Np, Nb)
    rc = 0.9 * cn.threshold_rc(3, DENSITY[3], cfg.Lbox)
    P = cn.random_paths(W, 2 * Nb + 1, Np, cfg.Lbox, np.random.default_rng(Np))
    P[1, 4] = P[1, 3]
    exp = pn.Window(P, Nb, window, cfg.Lbox, rc, 2 * window).expected([0, 1])
    assert np.all(exp["first"] > 0) and np.all(exp["both"][:, 1:] < exp["first"][:, 1:])
    _assert_same(_run(gpu_lib, cfg, P, rc, window, 2 * window, [None]), exp, f"lags at Np {Np}")


# ---- 5. contract ------------------------------------------------------------------------------------------------------
def _small():
    cfg = _cfg(3, 70, 3)
    return cfg, cn.random_paths(3, 7, 70, cfg.Lbox, np.random.default_rng(70)), 0.9 * cn.threshold_rc(3, DENSITY[3], cfg.Lbox)


def test_list_splits_and_a_walker_listed_twice(gpu_lib):
    cfg, P, rc = _small()
    whole = _run(gpu_lib, cfg, P, rc, 2, 3, [None])
    _same(_run(gpu_lib, cfg, P, rc, 2, 3, [[2], [1], [0]]), whole, "one by one")
    _same(_run(gpu_lib, cfg, P, rc, 2, 3, [[1, 0], [2]]), whole, "two and one")
    win = pn.Window(P, 3, 2, cfg.Lbox, rc, 3)
    exp = win.expected(range(3))
    assert np.any(exp["terms"] > 1) and exp["nwrap"][:, 1:].sum() > 0   # an order to keep, and wrapping clusters beside
    _assert_same(whole, exp, "whole")
    twice = _run(gpu_lib, cfg, P, rc, 2, 3, [[1, 1, 0]])
    _assert_same(twice, win.expected([1, 1, 0]), "listed twice")
    assert twice["samples"].tolist() == [5, 10, 0] and np.array_equal(twice["both"][1], 2 * whole["both"][1])


def test_scratch_budget_reset_and_init_again(gpu_lib):
    """A budget of 1 MiB holds fewer walkers than the list: more launches, the same bits.  Then the per-walker reset, and
    pc_init again, which resizes and zeroes."""
    Np, Nb, W = 300, 3, 70
    cfg = _cfg(2, Np, Nb)
    L = cfg.Lbox[:2]
    rc = 0.9 * cn.threshold_rc(2, DENSITY[2], L)
    P = np.broadcast_to(cn.random_paths(2, 2 * Nb + 1, Np, L, np.random.default_rng(5))[np.arange(W) % 2], (W, 7, Np, 2)).copy()
    assert (1 << 20) // (12 * 7 * Np) == 41 < W
    VT, WF = gpu_lib.build_tables(cfg)
    with gpu_lib.PigsContext(cfg, VT, WF, n_walkers=W) as ctx:
        ctx.upload_all(P)
        ctx.pc_init(rc, Nb, 2)
        ctx.pc_accumulate()
        whole = ctx.pc_read()
        ctx.set_tuning("pc_scratch_mib", 1)
        ctx.pc_init(rc, Nb, 2)
        ctx.pc_accumulate()
        split = ctx.pc_read(reset=[w == 1 for w in range(W)])
        again = ctx.pc_read()
        ARG = ST["PIGS_ERR_ARG"]
        assert ctx.L.pigs_set_tuning(ctx.h, b"pc_scratch_mib", 0) == ARG and ctx.L.pigs_set_tuning(ctx.h, b"pc_scratch_mib", 2049) == ARG
        ctx.pc_init(rc, 1, 1)
        fresh = ctx.pc_read()
    _same(split, whole, "budget")
    exp = pn.Window(P[:2], Nb, Nb, L, rc, 2).expected([0, 1])
    for k in INTS + ("rg2u", "terms"):
        exp[k] = exp[k][np.arange(W) % 2]
    _assert_same(whole, exp, "budget")
    keep = np.arange(W) != 1
    for k in INTS + ("rg2u",):
        assert np.array_equal(again[k][keep], split[k][keep]) and not np.any(again[k][1]), k
        assert not np.any(fresh[k]), k
    assert fresh["first"].shape == (W, 2) and (fresh["window"], fresh["ntau"]) == (1, 1)


def test_status_codes(gpu_lib):
    Nb = 3
    ARG, OK, UNS = ST["PIGS_ERR_ARG"], ST["PIGS_OK"], ST["PIGS_ERR_UNSUPPORTED"]
    cfg = _cfg(2, 30, Nb)
    half = 0.5 * min(cfg.Lbox[:2])
    VT, WF = gpu_lib.build_tables(cfg)
    with gpu_lib.PigsContext(cfg, VT, WF, n_walkers=2) as ctx:
        init = lambda rc, window, ntau: ctx.L.pigs_pc_init(ctx.h, C.c_double(rc), window, ntau)
        assert ctx.L.pigs_pc_accumulate(ctx.h, 1, None) == ARG              # before init
        with pytest.raises(gpu_lib.PigsError):
            ctx.pc_read()
        d, l = np.zeros(60), np.zeros(60, np.int64)
        dp, lp = d.ctypes.data_as(C.POINTER(C.c_double)), l.ctypes.data_as(C.POINTER(C.c_int64))
        assert ctx.L.pigs_pc_read(ctx.h, lp, lp, lp, lp, lp, dp, lp, lp, lp, lp, None) == ARG
        a, b = C.c_int32(0), C.c_int32(0)
        assert ctx.L.pigs_pc_sweeps(ctx.h, C.byref(a), C.byref(b)) == ARG
        for args in ((0.0, 0, 0), (-1.0, 0, 0), (float("nan"), 0, 0), (float("inf"), 0, 0),
                     (float(np.nextafter(half, np.inf)), 0, 0), (1.0, -1, 0), (1.0, Nb + 1, 0), (1.0, 1, -1), (1.0, 1, 3), (1.0, 0, 1)):
            assert init(*args) == ARG, args
            assert ctx.L.pigs_pc_accumulate(ctx.h, 1, None) == ARG
        assert init(half, 0, 0) == OK and init(1.0, Nb, 2 * Nb) == OK
        assert ctx.L.pigs_pc_accumulate(ctx.h, -1, None) == ARG
        assert ctx.L.pigs_pc_accumulate(ctx.h, 1, np.array([2], np.int32).ctypes.data_as(_ip)) == ARG
        assert ctx.L.pigs_pc_accumulate(ctx.h, 1, np.array([-1], np.int32).ctypes.data_as(_ip)) == ARG
        assert ctx.L.pigs_pc_accumulate(ctx.h, 0, None) == OK
        assert ctx.L.pigs_pc_read(ctx.h, lp, lp, lp, lp, lp, None, lp, lp, lp, lp, None) == ARG
        assert ctx.L.pigs_pc_sweeps(ctx.h, None, C.byref(b)) == ARG
        ctx.sync()
        assert ctx.L.pigs_pc_np_max() == ctx.L.pigs_cl_np_max()
    tcfg = SystemConfig(dim=2, Np=6, Nb=2, trap=True, a_ho=[1.0, 1.3], Nmax=2000, Rm=1.2, dt=0.01)
    VT, WF = gpu_lib.build_tables(tcfg)
    with gpu_lib.PigsContext(tcfg, VT, WF, n_walkers=1) as ctx:
        assert ctx.L.pigs_pc_init(ctx.h, C.c_double(0.5), 0, 0) == UNS
        assert ctx.L.pigs_pc_accumulate(ctx.h, 1, None) == ARG
        ctx.sync()


# ---- 6. the front end ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def exe(gpu_lib):
    import os
    import subprocess
    from conftest import ROOT
    host = os.path.join(ROOT, "pathintegralgroundstate_amd", "host")
    subprocess.check_call(["make", "-s", "-C", host])
    return os.path.join(host, "pigs_vpi")


def test_front_end_two_blocks_three_steps(gpu_lib, oracle, exe, tmp_path):
    """he4_cworm0 (2D, periodic, nine particles), 2 blocks x 3 steps, two walkers, percolation = T over a window of 2 with
    the lags 0..3: every file of the run without the key byte for byte; the three new files of every walker against a
    replay of the run's chains through PigsContext.pc_*."""
    import os
    import re
    from test_gpu_front_end_blocks import _input, _run as run_vpi, replay
    from test_pc_host import RAW, check_files
    run, W, Nblock, Nstep, window, ntau = "he4_cworm0", 2, 2, 3, 2, 3
    txt, cfg = _input(run, Nblock, Nstep)
    assert not cfg.trap and cfg.Nb >= window
    rc = 0.6 * cfg.rcut                                                 # test_gpu_cl.py's: singles beside bonded particles
    key = f", percolation = T, pc_rc = {rc!r}, pc_window = {window}, pc_ntau = {ntau}"
    rep = replay(gpu_lib, oracle, cfg, W, Nblock, Nstep)
    VT, WF = gpu_lib.build_tables(cfg)
    blocks = []
    with gpu_lib.PigsContext(cfg, VT, WF, n_walkers=W) as ctx:
        ctx.pc_init(rc, window, ntau)
        for b in range(Nblock):
            for t in range(b * Nstep, (b + 1) * Nstep):
                ctx.upload_all(rep["snaps"][t])
                wl = np.nonzero(rep["diag"][t])[0]
                if len(wl):
                    ctx.pc_accumulate(wl)
            blocks.append(ctx.pc_read(reset=True))
    counted = np.stack([b["samples"] > 0 for b in blocks], axis=1)           # [W, Nblock]
    assert counted.any() and sum(int(b["first"].sum()) for b in blocks) > 0
    assert sum(int(b["nfin"][:, 1:].sum()) for b in blocks) > 0             # finite clusters of several particles: percsz has lines
    plain, on = str(tmp_path / "plain"), str(tmp_path / "on")
    os.makedirs(plain), os.makedirs(on)
    run_vpi(exe, txt + f"&gpu\n n_walkers = {W}\n/\n", plain)
    out = run_vpi(exe, txt + f"&gpu\n n_walkers = {W}{key}\n/\n", on)
    assert "Percolation" in out and "perc_vpi.out" in out
    old = sorted(os.listdir(plain))
    new = sorted(set(os.listdir(on)) - set(old))
    assert sorted(f for f in new if ".w" not in f) == ["clpers_vpi.out", "perc_vpi.out", "percsz_vpi.out"], new
    assert len(new) == 3 + 3 * W, new
    for f in old:
        if f not in ("stdout.txt", "vpi.in"):
            assert open(os.path.join(plain, f), "rb").read() == open(os.path.join(on, f), "rb").read(), f
    names = sorted(f for f in new if re.fullmatch(r"perc_vpi\.w\d+\.out", f))
    assert len(names) == W
    checked = 0
    for w, fb in enumerate(names):
        bs = [b for b in range(Nblock) if counted[w, b]]
        if not bs:
            continue
        raws = [{k: blocks[b][k][w] for k in RAW} for b in bs]
        check_files(os.path.join(on, fb), os.path.join(on, fb.replace("perc_", "percsz_")),
                    os.path.join(on, fb.replace("perc_", "clpers_")), raws, cfg.Np, cfg.dim, cfg.dt, block_ids=[b + 1 for b in bs])
        checked += 1
    assert checked > 0
