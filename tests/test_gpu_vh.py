"""The van Hove histograms on the MI355X (pigs_vh_*, pigs_vh.hip) through the C ABI, against the numpy restatement in
tests/vh_numpy.py (pinned to closed forms by tests/test_vh_numpy_host.py).  Every count is an integer: every comparison is
exact equality over all elements.

Shapes: Np = 2, 3, 64, 65, 256, 257, 300 are the edges of a wave, of the 256 owners of a round, and of last rounds of one
and of 44 owners (which the kernel shares out over partner groups); each runs in 1D, 2D and 3D with Nb = 2 and 6, the
windows and lags (0,0), (1,1), (1,2), (Nb,0), (Nb,2Nb), the grids Nr = 1, 50 and Ns = 1, 40, and both kernel forms
(tuning key vh_form: histograms in LDS, global atomics) beside the automatic choice.  One case sits just past the
histogram size at which the automatic form leaves LDS, read from kVhLdsBudget, and one holds a slice of Np = 3000 in 3D
(72 000 bytes of LDS, which needs the launch header's grant)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import block_stats_numpy as bs
import vh_numpy
from conftest import ROOT
from pathintegralgroundstate_amd import SystemConfig
from vh_numpy import Window, n_pairs

pytestmark = pytest.mark.gpu
DENSITY = {1: 0.2, 2: 0.25, 3: 0.365}
FORMS = (0, 1, -1)


def _header():
    return open(os.path.join(ROOT, "include", "pigs_hip.h")).read()


ST = {k: int(v) for k, v in re.findall(r"^\s*(PIGS_\w+)\s*=\s*(-?\d+)", _header(), flags=re.M)}


def _lds_budget():
    """kVhLdsBudget of pigs_kernels.h, and the same number in the header's formulas."""
    txt = open(os.path.join(ROOT, "pathintegralgroundstate_amd", "csrc", "pigs_kernels.h")).read()
    a, b = re.search(r"constexpr\s+size_t\s+kVhLdsBudget\s*=\s*(\d+)\s*\*\s*(\d+)\s*;", txt).groups()
    n = int(a) * int(b)
    assert f"8 dim Np > {n}" in _header() and f"8 dim Np + 4 (Ntau + 1) (Nr + Ns) <= {n}" in _header()
    return n


LDS = _lds_budget()


def _cfg(dim, Np, Nb, **kw):
    return SystemConfig(dim=dim, Np=Np, Nb=Nb, density=DENSITY[dim], **kw)


def _random_paths(cfg, W, rng, scale=0.5):
    L = np.asarray(cfg.Lbox[:cfg.dim])
    return rng.uniform(-scale, scale, (W,) + tuple(cfg.path_shape)) * L


def _rbin(cfg, Nr):
    return cfg.rcut / float(np.float32(Nr))


def _sbin_cap(cfg, Ns):
    """A self grid that no once-folded displacement of in-box beads can leave: |d_k| <= L_k/2 after one fold of a
    difference of in-box coordinates, so |d| <= sqrt(dim) max_k L_k / 2 < Ns sbin."""
    return 1.01 * np.sqrt(cfg.dim) * max(cfg.Lbox[:cfg.dim]) / (2.0 * Ns)


def _same(got, exp, what):
    for k in ("samples", "self", "distinct"):
        assert got[k].dtype == np.int64 and got[k].shape == exp[k].shape, (what, k, got[k].shape, exp[k].shape)
        assert np.array_equal(got[k], exp[k]), (what, k, int(np.abs(got[k] - exp[k]).sum()))


def _fits(cfg, Ntau, Nr, Ns):
    return 8 * cfg.dim * cfg.Np + 4 * (Ntau + 1) * (Nr + Ns) <= LDS


def _each_form(gpu_lib, ctx, cfg, Ntau, Nr, Ns):
    """Sets every form in turn; a forced LDS form that does not fit is refused at the accumulate and skipped."""
    for form in FORMS:
        ctx.set_tuning("vh_form", form)
        if form == 1 and not _fits(cfg, Ntau, Nr, Ns):
            assert ctx.L.pigs_vh_accumulate(ctx.h, ctx.n_walkers, None) == ST["PIGS_ERR_ARG"]
            assert not ctx.vh_read()["samples"].any()                   # nothing was queued
            continue
        yield form
    ctx.set_tuning("vh_form", -1)


def _compare(gpu_lib, ctx, cfg, win, window, Ntau, Nr, Ns, what, walkers=None):
    """init on the capped self grid, one accumulate per form, the cap, the restatement, and lag 0 against pigs_grv_*."""
    rbin, sbin = _rbin(cfg, Nr), _sbin_cap(cfg, Ns)
    W = ctx.n_walkers
    wl = range(W) if walkers is None else walkers
    exp = win.expected(wl, Nr, rbin, Ns, sbin)
    ctx.vh_init(Ntau, window, Nr, rbin, Ns, sbin)
    for form in _each_form(gpu_lib, ctx, cfg, Ntau, Nr, Ns):
        ctx.vh_accumulate(walkers)
        got = ctx.vh_read(reset=True)
        tag = f"{what} W {window} Ntau {Ntau} Nr {Nr} Ns {Ns} form {form}"
        # the cap first, so that a dropping bug cannot hide behind the comparison
        cap = got["samples"][:, None] * n_pairs(window, Ntau)[None, :] * cfg.Np
        assert np.array_equal(got["self"].sum(axis=2), cap), (tag, got["self"].sum(axis=2), cap)
        _same(got, exp, tag)
        last = got
    # lag 0 of the device's counts against the device's pigs_grv_* on the same grid, window and worldline
    ctx.grv_init(2, window, Nr, rbin)
    ctx.grv_accumulate(walkers)
    assert np.array_equal(last["distinct"][:, 0], 2 * ctx.grv_read()["radial"]), what


# ---- 1. against the restatement on random in-box worldlines -----------------------------------------------------------
@pytest.mark.parametrize("Np", [2, 3, 64, 65, 256, 257, 300])
@pytest.mark.parametrize("dim", [1, 2, 3])
def test_matches_numpy_on_uploaded_worldlines(gpu_lib, dim, Np):
    W = 2
    for Nb in (2, 6):
        cfg = _cfg(dim, Np, Nb)
        VT, WF = gpu_lib.build_tables(cfg)
        P = _random_paths(cfg, W, np.random.default_rng(1000 * dim + 10 * Np + Nb))
        with gpu_lib.PigsContext(cfg, VT, WF, n_walkers=W) as ctx:
            ctx.upload_all(P)
            for window, Ntau in ((0, 0), (1, 1), (1, 2), (Nb, 0), (Nb, 2 * Nb)):
                win = Window(P, Nb, window, Ntau, cfg.Lbox, cfg.rcut2)
                for Nr, Ns in ((1, 1), (50, 40), (1, 40), (50, 1)):
                    _compare(gpu_lib, ctx, cfg, win, window, Ntau, Nr, Ns, f"dim {dim} Np {Np} Nb {Nb}")
                del win


@pytest.mark.parametrize("dim,Np,Ntau", [(1, 2, 0), (3, 65, 2)])
def test_histograms_just_past_the_lds_form(gpu_lib, dim, Np, Ntau):
    """The largest Nr whose histograms still sit in LDS beside the slice, and the next one, which takes global atomics:
    8 dim Np + 4 (Ntau + 1)(Nr + Ns) against kVhLdsBudget."""
    W, Nb, window, Ns = 2, 2, 1, 40
    cfg = _cfg(dim, Np, Nb)
    last = (LDS - 8 * dim * Np) // (4 * (Ntau + 1)) - Ns
    assert _fits(cfg, Ntau, last, Ns) and not _fits(cfg, Ntau, last + 1, Ns)
    VT, WF = gpu_lib.build_tables(cfg)
    P = _random_paths(cfg, W, np.random.default_rng(dim + Np))
    win = Window(P, Nb, window, Ntau, cfg.Lbox, cfg.rcut2)
    with gpu_lib.PigsContext(cfg, VT, WF, n_walkers=W) as ctx:
        ctx.upload_all(P)
        for Nr in (last, last + 1):
            _compare(gpu_lib, ctx, cfg, win, window, Ntau, Nr, Ns, f"threshold dim {dim} Np {Np}")


def test_slice_of_3000_particles_takes_the_lds_grant(gpu_lib):
    """Np = 3000 in 3D: the staged slice alone is 72 000 bytes, beyond what a kernel gets without a grant.  One walker,
    binned slice pair by slice pair (the r2 of a slice pair are 9 M doubles)."""
    dim, Np, Nb, window, Ntau, Nr, Ns = 3, 3000, 1, 1, 2, 50, 40
    cfg = _cfg(dim, Np, Nb)
    assert 8 * dim * Np > 64 * 1024
    VT, WF = gpu_lib.build_tables(cfg)
    P = _random_paths(cfg, 1, np.random.default_rng(3000))
    rbin, sbin = _rbin(cfg, Nr), _sbin_cap(cfg, Ns)
    off = ~np.eye(Np, dtype=bool)
    S, D = np.zeros((1, Ntau + 1, Ns), np.int64), np.zeros((1, Ntau + 1, Nr), np.int64)
    for l in range(Ntau + 1):
        for a in range(Nb - window, Nb + window - l + 1):
            r2 = vh_numpy.r2_matrix(P[0, a + l], P[0, a], cfg.Lbox)
            S[0, l] += vh_numpy.bin_self(np.diagonal(r2), Ns, sbin)
            D[0, l] += vh_numpy.bin_distinct(r2[off], cfg.rcut2, Nr, rbin)
    exp = {"self": S, "distinct": D, "samples": np.ones(1, np.int64)}
    with gpu_lib.PigsContext(cfg, VT, WF, n_walkers=1) as ctx:
        ctx.upload_all(P)
        ctx.vh_init(Ntau, window, Nr, rbin, Ns, sbin)
        for form in _each_form(gpu_lib, ctx, cfg, Ntau, Nr, Ns):
            ctx.vh_accumulate()
            got = ctx.vh_read(reset=True)
            assert np.array_equal(got["self"].sum(axis=2), n_pairs(window, Ntau)[None, :] * Np)
            _same(got, exp, f"Np 3000 form {form}")


# ---- 2. edges -------------------------------------------------------------------------------------------------------
def test_bin_edges_cutoff_and_coincident_particles_in_1d(gpu_lib):
    """1D, L = 32, rcut = 16, bins of width 1 (distinct) and 1/2 (self), every coordinate a multiple of 1/2: every u is an
    exact integer on both grids.  A pair sits exactly at r2 = rcut2 (counted: bin 16 of 20), two particles coincide
    (distinct bin 0), and the displacements along the path are multiples of 1/2 too."""
    Np, Nb, window, Ntau, Nr, Ns, W = 8, 3, 3, 6, 20, 12, 2
    cfg = SystemConfig(dim=1, Np=Np, Nb=Nb, density=0.25)
    assert cfg.Lbox[0] == 32.0 and cfg.rcut2 == 256.0
    rng = np.random.default_rng(11)
    base = np.array([-12.0, 4.0, 4.0, -3.5, 9.5, 0.0, 15.5, -15.5])           # 0-1: 16 apart; 1-2 coincide
    P = np.empty((W, 2 * Nb + 1, Np, 1))
    for w in range(W):
        P[w, :, :, 0] = base + 0.5 * np.cumsum(rng.integers(-1, 2, (2 * Nb + 1, Np)), axis=0)
    P[:, :, :3, 0] = base[:3]                                                # these three stay put
    win = Window(P, Nb, window, Ntau, cfg.Lbox, cfg.rcut2)
    exp = win.expected(range(W), Nr, 1.0, Ns, 0.5)
    assert np.all(exp["distinct"][:, :, 16] >= 2 * n_pairs(window, Ntau)) and np.all(exp["distinct"][:, :, 0] >= 2 * n_pairs(window, Ntau))
    assert exp["distinct"][:, :, 17:].sum() == 0 and exp["self"][:, 1:, 1:].sum() > 0
    VT, WF = gpu_lib.build_tables(cfg)
    with gpu_lib.PigsContext(cfg, VT, WF, n_walkers=W) as ctx:
        ctx.upload_all(P)
        ctx.vh_init(Ntau, window, Nr, 1.0, Ns, 0.5)
        for form in _each_form(gpu_lib, ctx, cfg, Ntau, Nr, Ns):
            ctx.vh_accumulate()
            _same(ctx.vh_read(reset=True), exp, f"1D edges form {form}")


@pytest.mark.parametrize("dim,Np", [(1, 9), (2, 70), (3, 257)])
def test_degenerate_inputs_drop_out_as_in_numpy(gpu_lib, dim, Np):
    """A bead far outside the box, NaN and +-Inf coordinates: walker 0 has them, walker 1 is clean and keeps its counts."""
    Nb, window, Ntau, W, Nr, Ns = 3, 2, 3, 2, 30, 20
    cfg = _cfg(dim, Np, Nb)
    VT, WF = gpu_lib.build_tables(cfg)
    clean = _random_paths(cfg, W, np.random.default_rng(5 * dim))
    P = clean.copy()
    L = np.asarray(cfg.Lbox[:dim])
    P[0, Nb, 2, 0] = np.nan
    P[0, Nb - 1, 3, dim - 1] = np.inf
    P[0, Nb + 1, 4] = -np.inf
    P[0, :, 5] = 7.3 * L                                                     # one fold leaves it far outside
    P[0, Nb, 6] = -7.3 * L                                                   # a displacement that one fold leaves far outside
    rbin, sbin = _rbin(cfg, Nr), _sbin_cap(cfg, Ns)
    with gpu_lib.PigsContext(cfg, VT, WF, n_walkers=W) as ctx:
        ctx.vh_init(Ntau, window, Nr, rbin, Ns, sbin)
        for form in _each_form(gpu_lib, ctx, cfg, Ntau, Nr, Ns):
            ctx.upload_all(clean)
            ctx.vh_accumulate()
            ref = ctx.vh_read(reset=True)
            ctx.upload_all(P)
            ctx.vh_accumulate()
            got = ctx.vh_read(reset=True)
            exp = Window(P, Nb, window, Ntau, cfg.Lbox, cfg.rcut2).expected(range(W), Nr, rbin, Ns, sbin)
            _same(got, exp, f"degenerate dim {dim} form {form}")
            for k in ("self", "distinct"):
                assert np.array_equal(got[k][1], ref[k][1]), k
            assert got["self"][0].sum() < ref["self"][0].sum() and got["distinct"][0].sum() < ref["distinct"][0].sum()


@pytest.mark.parametrize("dim", [2, 3])
def test_box_with_unequal_sides(gpu_lib, dim):
    Np, Nb, W = 65, 4, 2
    L = (Np / DENSITY[dim]) ** (1.0 / dim)
    cfg = _cfg(dim, Np, Nb, Lbox=[0.8 * L, 1.25 * L] if dim == 2 else [0.8 * L, 1.25 * L, L])
    VT, WF = gpu_lib.build_tables(cfg)
    P = _random_paths(cfg, W, np.random.default_rng(77 + dim))
    with gpu_lib.PigsContext(cfg, VT, WF, n_walkers=W) as ctx:
        ctx.upload_all(P)
        _compare(gpu_lib, ctx, cfg, Window(P, Nb, 3, 4, cfg.Lbox, cfg.rcut2), 3, 4, 50, 40, f"unequal sides dim {dim}")


# ---- 3. invariance --------------------------------------------------------------------------------------------------
def test_counts_do_not_depend_on_the_list_or_the_split(gpu_lib):
    """257 walkers of Np = 2: one call (two launches, split at 256) against two calls, a reversed list, a walker listed
    three times, the reset mask and a second init."""
    W, Np, dim, Nb, window, Ntau, Nr, Ns = 257, 2, 3, 2, 2, 3, 6, 5
    cfg = _cfg(dim, Np, Nb)
    VT, WF = gpu_lib.build_tables(cfg)
    P = _random_paths(cfg, W, np.random.default_rng(9))
    rbin, sbin = _rbin(cfg, Nr), _sbin_cap(cfg, Ns)
    win = Window(P, Nb, window, Ntau, cfg.Lbox, cfg.rcut2)
    with gpu_lib.PigsContext(cfg, VT, WF, n_walkers=W) as ctx:
        ctx.upload_all(P)
        ctx.vh_init(Ntau, window, Nr, rbin, Ns, sbin)
        for form in _each_form(gpu_lib, ctx, cfg, Ntau, Nr, Ns):
            ctx.vh_accumulate()
            whole = ctx.vh_read(reset=True)
            _same(whole, win.expected(range(W), Nr, rbin, Ns, sbin), f"257 walkers form {form}")
            ctx.vh_accumulate(list(range(100)))
            ctx.vh_accumulate(list(range(100, W)))
            _same(ctx.vh_read(reset=True), whole, "two calls")
            ctx.vh_accumulate(list(range(W - 1, -1, -1)))
            _same(ctx.vh_read(reset=True), whole, "reversed list")
            wl = [7, 3, 7, 256, 7]
            ctx.vh_accumulate(wl)
            twice = ctx.vh_read()
            _same(twice, win.expected(wl, Nr, rbin, Ns, sbin), "a walker listed three times")
            assert np.array_equal(twice["distinct"][7], 3 * whole["distinct"][7]) and twice["samples"][7] == 3
            # reset zeroes only the walkers named
            mask = np.zeros(W, np.int32)
            mask[[3, 256]] = 1
            ctx.vh_read(reset=mask)
            after = ctx.vh_read(reset=True)
            assert after["samples"].sum() == 3 and after["samples"][7] == 3 and not after["self"][[3, 256]].any()
            assert np.array_equal(after["self"][7], twice["self"][7]) and np.array_equal(after["distinct"][7], twice["distinct"][7])
        # a second init resizes and zeroes, also with a call in flight
        ctx.vh_accumulate()
        ctx.vh_init(1, 1, 3, rbin, 2, sbin)
        z = ctx.vh_read()
        assert z["self"].shape == (W, 2, 2) and z["distinct"].shape == (W, 2, 3) and not any(z[k].any() for k in z)
        ctx.vh_accumulate([5])
        _same(ctx.vh_read(), Window(P, Nb, 1, 1, cfg.Lbox, cfg.rcut2).expected([5], 3, rbin, 2, sbin), "after re-init")
    # another context with one walker: the same worldline, the same counts
    with gpu_lib.PigsContext(cfg, VT, WF, n_walkers=1) as one:
        one.upload_all(P[5:6])
        one.vh_init(Ntau, window, Nr, rbin, Ns, sbin)
        one.vh_accumulate()
        got = one.vh_read()
        for k in ("self", "distinct", "samples"):
            assert np.array_equal(got[k][0], whole[k][5]), k


# ---- 4. after the sampler ---------------------------------------------------------------------------------------------
RUNS = os.path.join(ROOT, "tests", "golden", "vpi_runs")


def _chain(gpu_lib, oracle, cfg, W, steps, vh=None):
    """`steps` MC steps of W chains as the front end starts them; vh = (Ntau, window, Nr, rbin, Ns, sbin): an accumulate
    queued behind every step, with no synchronisation in between.  (worldlines after every step, final, vh_read)."""
    from oracle.pyoracle import System
    S = System(dim=cfg.dim, Np=cfg.Np, Nb=cfg.Nb, density=cfg.density, dt=cfg.dt, trap=cfg.trap, a_ho=cfg.a_ho,
               Lbox=cfg.Lbox, rcut=cfg.rcut)
    VT, WF = gpu_lib.build_tables(cfg)
    with gpu_lib.PigsContext(cfg, VT, WF, n_walkers=W) as ctx:
        ctx.sampler_init(CWorm=cfg.CWorm, swapping=cfg.swapping, Nobdm=cfg.Nobdm, Nbin=cfg.Nbin, Npw=cfg.Npw,
                         sampling=cfg.sampling)
        P0, xend = [], []
        for w in range(W):
            P, g = oracle.init_path(S, cfg.seed + w)
            P0.append(P)
            xend.append(np.stack([P[cfg.Nb, cfg.Np - 1], P[cfg.Nb, cfg.Np - 1]]))
            ctx.sampler_set_rng(w, g.mti, np.array(g.mt[:], np.uint32))
        ctx.upload_all(np.stack(P0))
        ctx.sampler_set_worm(np.zeros(W, np.int32), np.zeros(W, np.int32), np.stack(xend))
        snaps = []
        if vh is not None:
            ctx.vh_init(*vh)
        for istep in range(1, steps + 1):
            ctx.sampler_step(istep)
            if vh is not None:
                ctx.vh_accumulate()
            else:
                snaps.append(ctx.download_all())
        return snaps, ctx.download_all(), (ctx.vh_read() if vh is not None else None)


def test_accumulate_behind_sampler_steps_with_swaps(gpu_lib, oracle):
    """he4_wormbusy_s7 (3D, worm and swap moves on): the counts queued behind every step are the restatement's on the
    worldlines a twin chain downloads after the same steps, and the family leaves the worldlines bit-identical."""
    cfg = SystemConfig.from_namelists(open(os.path.join(RUNS, "he4_wormbusy_s7", "vpi.in")).read())
    assert cfg.swapping and cfg.CWorm > 0 and not cfg.trap
    W, steps, Ntau, window, Nr, Ns = 3, 12, 4, 3, cfg.Nbin, 30
    rbin, sbin = _rbin(cfg, Nr), 0.05
    snaps, final_plain, _ = _chain(gpu_lib, oracle, cfg, W, steps)
    _, final_vh, got = _chain(gpu_lib, oracle, cfg, W, steps, (Ntau, window, Nr, rbin, Ns, sbin))
    assert np.array_equal(final_plain, final_vh) and np.array_equal(final_plain, snaps[-1])
    exp = None
    for Pn in snaps:
        e = Window(Pn, cfg.Nb, window, Ntau, cfg.Lbox, cfg.rcut2).expected(range(W), Nr, rbin, Ns, sbin)
        exp = e if exp is None else {k: exp[k] + e[k] for k in e}
    _same(got, exp, "behind sampler_step")
    assert got["self"][:, 1:, 1:].sum() > 0                                  # the beads move along the path


# ---- 5. refusals ----------------------------------------------------------------------------------------------------
def test_status_codes(gpu_lib):
    W, Nb = 2, 3
    ARG, OK, UNS = ST["PIGS_ERR_ARG"], ST["PIGS_OK"], ST["PIGS_ERR_UNSUPPORTED"]
    assert len({ARG, OK, UNS}) == 3
    cfg = _cfg(2, 30, Nb)
    VT, WF = gpu_lib.build_tables(cfg)
    l = np.zeros(1 << 16, np.int64).ctypes.data_as(C.POINTER(C.c_int64))
    nan, inf = float("nan"), float("inf")
    with gpu_lib.PigsContext(cfg, VT, WF, n_walkers=W) as ctx:
        ctx.upload_all(_random_paths(cfg, W, np.random.default_rng(2)))
        init = lambda *a: ctx.L.pigs_vh_init(ctx.h, *a)
        with pytest.raises(gpu_lib.PigsError):
            ctx.vh_accumulate()
        with pytest.raises(gpu_lib.PigsError):
            ctx.vh_read()
        assert ctx.L.pigs_vh_accumulate(ctx.h, 1, None) == ARG and ctx.L.pigs_vh_read(ctx.h, l, l, l, None) == ARG
        for Ntau, window, Nr, rbin, Ns, sbin in ((0, 0, 0, 0.1, 5, 0.1), (0, 0, -1, 0.1, 5, 0.1), (0, 0, 5, 0.1, 0, 0.1),
                                                 (0, 0, 5, 0.0, 5, 0.1), (0, 0, 5, -0.1, 5, 0.1), (0, 0, 5, nan, 5, 0.1),
                                                 (0, 0, 5, inf, 5, 0.1), (0, 0, 5, 0.1, 5, 0.0), (0, 0, 5, 0.1, 5, -1.0),
                                                 (0, 0, 5, 0.1, 5, nan), (0, 0, 5, 0.1, 5, inf), (0, -1, 5, 0.1, 5, 0.1),
                                                 (0, Nb + 1, 5, 0.1, 5, 0.1), (-1, 1, 5, 0.1, 5, 0.1), (3, 1, 5, 0.1, 5, 0.1),
                                                 (1, 0, 5, 0.1, 5, 0.1),
                                                 (0, 0, 2 ** 27, 0.1, 1, 0.1), (0, 0, 1, 0.1, 2 ** 27, 0.1)):   # over 2 GiB
            assert init(Ntau, window, Nr, rbin, Ns, sbin) == ARG, (Ntau, window, Nr, rbin, Ns, sbin)
            with pytest.raises(gpu_lib.PigsError):
                ctx.vh_init(Ntau, window, Nr, rbin, Ns, sbin)
        assert ctx.L.pigs_vh_accumulate(ctx.h, 1, None) == ARG             # init stays undone
        # the limits themselves are accepted
        assert init(2 * Nb, Nb, 1, 1e-300, 1, 1e300) == OK
        ctx.vh_init(2 * Nb, Nb, 1, 1e-300, 1, 1e300)
        for bad in ([2], [-1], [0, 2]):
            with pytest.raises(gpu_lib.PigsError):
                ctx.vh_accumulate(bad)
        assert ctx.L.pigs_vh_accumulate(ctx.h, -1, None) == ARG
        assert ctx.L.pigs_vh_read(ctx.h, None, l, l, None) == ARG and ctx.L.pigs_vh_read(ctx.h, l, None, l, None) == ARG
        assert ctx.L.pigs_set_tuning(ctx.h, b"vh_form", 2) == ARG and ctx.L.pigs_set_tuning(ctx.h, b"vh_form", -2) == ARG
        assert ctx.L.pigs_vh_accumulate(ctx.h, W, None) == OK
        assert ctx.vh_read()["samples"].tolist() == [1] * W               # the refused lists added nothing
    # the slice has to fit the LDS: 8 dim Np against the budget, the formula of the header
    for Np, want in ((LDS // 24, OK), (LDS // 24 + 1, ARG)):
        big = _cfg(3, Np, 1)
        assert (8 * 3 * Np > LDS) == (want == ARG)
        VT, WF = gpu_lib.build_tables(big)
        with gpu_lib.PigsContext(big, VT, WF, n_walkers=1) as ctx:
            assert ctx.L.pigs_vh_init(ctx.h, 0, 0, 10, 0.1, 10, 0.1) == want, Np
    # trapped contexts: unsupported, a status of its own
    tcfg = SystemConfig(dim=2, Np=6, Nb=2, trap=True, a_ho=[1.0, 1.3], Nmax=2000, Rm=1.2, dt=0.01)
    VT, WF = gpu_lib.build_tables(tcfg)
    with gpu_lib.PigsContext(tcfg, VT, WF, n_walkers=1) as ctx:
        assert ctx.L.pigs_vh_init(ctx.h, 0, 0, 10, 0.1, 5, 0.1) == UNS
        assert ctx.L.pigs_vh_accumulate(ctx.h, 1, None) == ARG            # still before init
        with pytest.raises(gpu_lib.PigsError, match="periodic"):
            ctx.vh_init(0, 0)
        ctx.sync()                                                        # the context still works


# ---- 6. the front end -------------------------------------------------------------------------------------------------
PRINT = 1.0000001e-9            # the files carry 10 significant digits


@pytest.fixture(scope="module")
def exe(gpu_lib):
    import subprocess
    host = os.path.join(ROOT, "pathintegralgroundstate_amd", "host")
    subprocess.check_call(["make", "-s", "-C", host])
    return os.path.join(host, "pigs_vpi")


def _check_table(path, bv, counted, w, tau, r, what):
    """One gd/gs file (tau_l, r, mean, error per (lag, bin)) against the block values bv [W, Nblock, nl, n]."""
    nl, n = bv.shape[2:]
    tab = np.loadtxt(path)
    assert tab.shape == (nl * n, 4), (what, tab.shape)
    assert np.allclose(tab[:, 0], np.repeat(tau, n), rtol=PRINT, atol=0) and np.allclose(tab[:, 1], np.tile(r, nl), rtol=PRINT, atol=0)
    flat = bv.reshape(bv.shape[:2] + (-1,))
    mean, err, nb = bs.walker_stats(flat, counted, w) if w is not None else bs.average_stats(flat, counted)
    assert nb == bv.shape[1]
    mtol = PRINT * np.abs(mean)
    assert np.all(np.abs(tab[:, 2] - mean) <= mtol), (what, np.abs(tab[:, 2] - mean).max())
    etol = np.sqrt(4.0 * np.abs(mean) * mtol) + PRINT * np.abs(err)
    nan = np.isnan(tab[:, 3])
    assert not np.any(nan & (err > etol)) and np.all(np.abs(tab[:, 3] - err)[~nan] <= etol[~nan]), what
    assert np.any(err > etol) and mean.any(), (what, "no well-conditioned error bar: the check has no teeth")


def test_front_end_two_walkers_three_blocks(gpu_lib, oracle, exe, tmp_path):
    """he4_cworm0 (2D, CWorm = 0: every step is a diagonal one) with two walkers, gr_vector on in both runs and van_hove
    on in one: the old files byte for byte, gd_vpi.out / gs_vpi.out per walker and averaged against a replay of the run's
    chains (test_gpu_front_end_blocks.replay) through PigsContext.vh_* and normalize_vh, the lag 0 of gd_vpi.out against
    grw_vpi.out, and the same run on two shards of one device."""
    from pathintegralgroundstate_amd.profiles import normalize_vh
    from test_gpu_front_end_blocks import _input, _run as run_vpi, replay
    W, Nblock, Nstep, Ntau, window, Ns, rself = 2, 3, 2, 3, 2, 12, 1.5
    txt, cfg = _input("he4_cworm0", Nblock, Nstep)
    grv = f"n_walkers = {W}, gr_vector = T, gr_nbin = 4, gr_window = {window}"
    vh = f", van_hove = T, vh_ntau = {Ntau}, vh_window = {window}, vh_nself = {Ns}, vh_rself = {rself}"
    plain, on, sharded = str(tmp_path / "plain"), str(tmp_path / "on"), str(tmp_path / "sharded")
    run_vpi(exe, txt + f"&gpu\n {grv}\n/\n", plain)
    out = run_vpi(exe, txt + f"&gpu\n {grv}{vh}\n/\n", on)
    assert "Van Hove" in out
    old = sorted(os.listdir(plain))
    new = sorted(set(os.listdir(on)) - set(old))
    assert sorted(f for f in new if ".w" not in f) == ["gd_vpi.out", "gs_vpi.out"] and len(new) == 2 + 2 * W, new
    for f in old:
        if f not in ("stdout.txt", "vpi.in"):
            assert open(os.path.join(plain, f), "rb").read() == open(os.path.join(on, f), "rb").read(), f
    assert {"e_vpi.out", "gr_vpi.out", "sk_vpi.out", "grw_vpi.out"} <= set(old)
    # the replay IS the run
    rep = replay(gpu_lib, oracle, cfg, W, Nblock, Nstep)
    final = np.fromfile(os.path.join(on, "worldlines_final.bin")).reshape(rep["final"].shape)
    assert np.array_equal(final, rep["final"]) and rep["diag"].all()
    # block values through the C ABI and the package's normalisation
    sbin = rself / Ns
    VT, WF = gpu_lib.build_tables(cfg)
    Gd = np.zeros((W, Nblock, Ntau + 1, cfg.Nbin))
    Gs = np.zeros((W, Nblock, Ntau + 1, Ns))
    with gpu_lib.PigsContext(cfg, VT, WF, n_walkers=W) as ctx:
        ctx.vh_init(Ntau, window, cfg.Nbin, cfg.rbin, Ns, sbin)
        for b in range(Nblock):
            for P in rep["snaps"][b * Nstep:(b + 1) * Nstep]:
                ctx.upload_all(P)
                ctx.vh_accumulate()
            n = normalize_vh(ctx.vh_read(reset=True), cfg.Np, window, cfg.density, cfg.rbin, sbin, cfg.dim, cfg.dt)
            Gd[:, b], Gs[:, b] = n["G_d"], n["G_s"]
    assert not np.array_equal(Gd[0, 0], Gd[0, 1])                            # the blocks differ: the errors have teeth
    counted = np.ones((W, Nblock), bool)
    per_walker = sorted(f for f in new if re.fullmatch(r"gd_vpi\.w\d+\.out", f))
    assert len(per_walker) == W
    for w, f in enumerate(per_walker):
        _check_table(os.path.join(on, f), Gd, counted, w, n["tau"], n["r"], f)
        _check_table(os.path.join(on, f.replace("gd_", "gs_")), Gs, counted, w, n["tau"], n["rs"], f.replace("gd_", "gs_"))
    _check_table(os.path.join(on, "gd_vpi.out"), Gd, counted, None, n["tau"], n["r"], "gd_vpi.out")
    _check_table(os.path.join(on, "gs_vpi.out"), Gs, counted, None, n["tau"], n["rs"], "gs_vpi.out")
    # lag 0 of gd_vpi.out carries grw_vpi.out's printed r and G (equal windows)
    gd = [ln.split() for ln in open(os.path.join(on, "gd_vpi.out")) if ln.strip()]
    grw = [ln.split() for ln in open(os.path.join(on, "grw_vpi.out")) if ln.strip()]
    assert len(grw) == cfg.Nbin and [r[1:3] for r in gd[:cfg.Nbin]] == [r[0:2] for r in grw]
    assert any(float(r[1]) > 0 for r in grw)
    # two shards on one device: the averaged files equal the one-shard run's
    run_vpi(exe, txt + f"&gpu\n {grv}{vh}, device = 0, n_gpus = 2, same_device = T\n/\n", sharded)
    for f in ("gd_vpi.out", "gs_vpi.out"):
        a, b = np.loadtxt(os.path.join(on, f)), np.loadtxt(os.path.join(sharded, f))
        assert a.shape == b.shape and np.allclose(a[:, :3], b[:, :3], rtol=PRINT, atol=0), f
        # the shards' block values are added in another order (the all-reduce), so the means may differ in their last
        # printed digit; the error column is the root of a difference of two moments, which carries that digit as
        # sqrt(4 |mean| PRINT |mean|) -- the bound of every error column of this suite -- beside its own printed digits
        etol = np.sqrt(4.0 * np.abs(a[:, 2]) * PRINT * np.abs(a[:, 2])) + PRINT * np.abs(a[:, 3])
        both_nan = np.isnan(a[:, 3]) & np.isnan(b[:, 3])
        assert np.all(both_nan | (np.abs(a[:, 3] - b[:, 3]) <= etol)), f
