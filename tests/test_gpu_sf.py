"""The centre-of-mass diffusion along tau and the unfolded displacement on the MI355X (pigs_sf_*, pigs_sf.hip), through the
C ABI.

The expected sums come from the numpy restatement in tests/sf_numpy.py (the same IEEE operations in the same order; pinned
to a literal loop, to closed forms and to the free gas by tests/test_sf_numpy_host.py).  nwrap and samples must be EQUAL,
C of a single call must have the restatement's bits, and D lies within 1e-12 * Sum|terms| per element, the project's bound
for a fixed-order sum (tests/test_gpu_lat.py, tests/test_gpu_atm.py): every term is a square, so Sum|terms| is the expected
value itself.  No comparison masks or skips elements.  The worldlines are random walks in a box of unequal sides, wrapped
into the cell, so that links cross the faces.

Largest |got - want| / bound seen on the MI355X: see DESIGN.md (the superfluid section)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import sf_numpy as sn
from conftest import ROOT
from helpers import same_bits
from pathintegralgroundstate_amd import SystemConfig
from pathintegralgroundstate_amd.profiles import normalize_sf

pytestmark = pytest.mark.gpu
DENSITY = {1: 0.3, 2: 0.25, 3: 0.365}
_ip = C.POINTER(C.c_int32)


def _header():
    return open(os.path.join(ROOT, "include", "pigs_hip.h")).read()


ST = {k: int(v) for k, v in re.findall(r"^\s*(PIGS_\w+)\s*=\s*(-?\d+)", _header(), flags=re.M)}
assert ST["PIGS_OK"] == 0 and len({ST["PIGS_ERR_ARG"], ST["PIGS_ERR_HIP"], ST["PIGS_ERR_UNSUPPORTED"]}) == 3


def _cfg(dim, Np, Nb):
    """A box of unequal sides."""
    L = (Np / DENSITY[dim]) ** (1.0 / dim)
    return SystemConfig(dim=dim, Np=Np, Nb=Nb, density=DENSITY[dim], Lbox=[[L], [0.8 * L, 1.25 * L], [0.8 * L, 1.25 * L, L]][dim - 1])


def _dyadic(dim, Np, Nb):
    """A box of dyadic, unequal sides: with coordinates on the 2^-16 grid every operation of the family is exact."""
    Lbox = [8.0, 16.0, 4.0][:dim]
    return SystemConfig(dim=dim, Np=Np, Nb=Nb, density=Np / float(np.prod(Lbox)), Lbox=Lbox)


def _assert_same(got, exp, what):
    for k in ("nwrap", "samples"):
        assert got[k].dtype == np.int64 and got[k].shape == exp[k].shape, (what, k)
        assert np.array_equal(got[k], exp[k]), (what, k, got[k], exp[k])
    for k in ("C", "D"):
        assert got[k].shape == exp[k].shape and got[k].dtype == np.float64, (what, k)
    assert same_bits(got["C"], exp["C"]), (what, "C", float(np.nanmax(np.abs(got["C"] - exp["C"]))))
    assert np.array_equal(np.isnan(got["D"]), np.isnan(exp["D"])), (what, "D: NaN elsewhere")
    fin = ~np.isnan(exp["D"])
    bound = 1e-12 * np.abs(exp["D"][fin])
    err = np.abs(got["D"][fin] - exp["D"][fin])
    with np.errstate(all="ignore"):
        worst = float(np.max(np.where(err == 0, 0.0, err / bound), initial=0.0))
    print(f"{what}: max |got-want|/bound of D = {worst:.3e} over {err.size} elements")
    assert np.all(err <= bound), (what, worst)


def _run(gpu_lib, cfg, P, Ntau, window, lists, also=None):
    VT, WF = gpu_lib.build_tables(cfg)
    with gpu_lib.PigsContext(cfg, VT, WF, n_walkers=P.shape[0]) as ctx:
        ctx.upload_all(P)
        ctx.sf_init(Ntau, window)
        for wl in lists:
            ctx.sf_accumulate(wl)
        got = ctx.sf_read()
        return (got, also(ctx)) if also else got


def _fqs_D(ctx, Ntau, window):
    ctx.fqs_init(1, Ntau, window)
    ctx.fqs_accumulate()
    return ctx.fqs_read()["D"]


# ---- 1. against the numpy restatement -----------------------------------------------------------------------------------
@pytest.mark.parametrize("Np", [3, 64, 65, 257, 300])
@pytest.mark.parametrize("dim", [1, 2, 3])
def test_matches_numpy(gpu_lib, dim, Np):
    """Windows 0, 1 and Nb, each with Ntau = 0 and 2 window, on one context (sf_init again resizes and zeroes)."""
    Nb, W = 3, 2
    cfg = _cfg(dim, Np, Nb)
    P = sn.random_walk(W, 2 * Nb + 1, Np, cfg.Lbox[:dim], np.random.default_rng(1000 * dim + Np), 0.04)
    VT, WF = gpu_lib.build_tables(cfg)
    with gpu_lib.PigsContext(cfg, VT, WF, n_walkers=W) as ctx:
        ctx.upload_all(P)
        for window in (0, 1, Nb):
            for Ntau in sorted({0, 2 * window}):
                exp = sn.Window(P, Nb, window, cfg.Lbox[:dim], Ntau).expected(range(W))
                assert window < Nb or exp["nwrap"].sum() > 0, "no link of the window crosses a face"
                ctx.sf_init(Ntau, window)
                ctx.sf_accumulate()
                got = ctx.sf_read()
                assert got["window"] == window
                _assert_same(got, exp, f"dim {dim} Np {Np} window {window} Ntau {Ntau}")
                assert not np.any(got["C"][:, 0]) and not np.any(got["D"][:, 0]) and np.all(got["D"][:, 1:] > 0)


def test_large_system(gpu_lib):
    """Np = 1077 in 3D: five rounds of particles."""
    Np, Nb = 1077, 1
    cfg = _cfg(3, Np, Nb)
    P = sn.random_walk(1, 3, Np, cfg.Lbox, np.random.default_rng(1077), 0.04)
    exp = sn.Window(P, Nb, 1, cfg.Lbox, 2).expected([0])
    assert exp["nwrap"][0] > 0
    _assert_same(_run(gpu_lib, cfg, P, 2, 1, [None]), exp, "Np 1077")


# ---- 2. what the fold-once family cannot do, and where the two agree -----------------------------------------------------
@pytest.mark.parametrize("dim", [1, 2, 3])
def test_unfolding_beyond_half_the_box(gpu_lib, dim):
    """Every particle drifts 0.3 L per link (on the 2^-16 grid, dyadic sides: every operation is exact) over a window of
    nine slices: 2.4 L in all.  C and D equal the closed form bit for bit; pigs_fqs_*'s D, which folds the displacement
    once, falls short from the second lag on."""
    Np, Nb = 65, 4
    cfg = _dyadic(dim, Np, Nb)
    L = np.asarray(cfg.Lbox[:dim])
    c = np.round(0.3 * L * 64.0) / 64.0                                 # on the grid, and short enough for exact squares
    ns, Ntau = 2 * Nb + 1, 2 * Nb
    P = sn.drift(Np, ns, L, c, np.ones(Np), np.random.default_rng(dim))
    assert np.all(2 * c > 0.5 * L) and np.all(c < 0.5 * L) and np.all(Ntau * c > 2 * L)
    lags = np.arange(Ntau + 1.0)
    npairs = ns - lags
    wantC = npairs[:, None] * (Np * lags[:, None] * c) ** 2
    wantD = Np * npairs[:, None] * (lags[:, None] * c) ** 2
    exp = sn.Window(P, Nb, Nb, L, Ntau).expected([0])
    assert same_bits(exp["C"][0], wantC) and same_bits(exp["D"][0], wantD) and exp["nwrap"][0] > 0
    got, fD = _run(gpu_lib, cfg, P, Ntau, Nb, [None], also=lambda ctx: _fqs_D(ctx, Ntau, Nb))
    assert same_bits(got["C"][0], wantC) and same_bits(got["D"][0], wantD)
    assert got["nwrap"].tolist() == exp["nwrap"].tolist() and got["samples"].tolist() == [1]
    total = got["D"][0].sum(axis=1)
    assert fD[0, 1, 0] == total[1] and np.all(fD[0, 2:, 0] < total[2:]), (fD[0, :, 0], total)


@pytest.mark.parametrize("dim", [1, 2, 3])
def test_agrees_with_fqs_below_half_the_box(gpu_lib, dim):
    """Random steps on the 2^-16 grid whose sum over the window stays below L/2 per axis: the once-folded displacement is
    the unfolded one, every sum is exact, and sum_k D_sf[l][k] equals pigs_fqs_*'s D[l][0]."""
    Np, Nb, W = 65, 3, 2
    cfg = _dyadic(dim, Np, Nb)
    L = np.asarray(cfg.Lbox[:dim])
    rng = np.random.default_rng(20 + dim)
    step = sn.on_grid(rng.uniform(-0.07, 0.07, (W, 2 * Nb + 1, Np, dim)) * L)
    path = np.cumsum(step, axis=1)
    assert np.all(np.abs(path - path[:, :1]).max(axis=1) < 0.5 * L - 0.01)
    P = sn.wrap(sn.on_grid(rng.uniform(-0.5, 0.5, (W, 1, Np, dim)) * L) + path, L)
    exp = sn.Window(P, Nb, Nb, L, 2 * Nb).expected(range(W))
    assert np.all(exp["nwrap"] > 0)
    got, fD = _run(gpu_lib, cfg, P, 2 * Nb, Nb, [None], also=lambda ctx: _fqs_D(ctx, 2 * Nb, Nb))
    _assert_same(got, exp, f"below L/2, dim {dim}")
    assert same_bits(got["D"], exp["D"])
    assert np.array_equal(got["D"].sum(axis=2), fD[..., 0]) and np.all(fD[:, 1:, 0] > 0)


def test_a_wrap_at_the_face_and_a_link_of_exactly_half_the_box(gpu_lib):
    """Particle 0 crosses the face at +L_x/2 and comes back one link later: two folds, and its unfolded path returns to 0.
    Particle 1 moves by exactly +L_x/2 and back: the compares are strict, so neither link is folded or counted."""
    cfg = _dyadic(2, 3, 2)
    X = np.zeros((5, 3, 2))
    X[:, 0, 0] = [3.75, -3.75, 3.75, 3.75, 3.75]
    X[:, 1, 0] = [-2.0, 2.0, -2.0, -2.0, -2.0]
    X[:, 2] = [1.0, -5.0]
    P = X[None].copy()
    d, U, Wc, nwrap = sn.unfold(P[0], cfg.Lbox[:2])
    assert nwrap == 2 and U[:, 0, 0].tolist() == [0.0, 0.5, 0.0, 0.0, 0.0] and U[:, 1, 0].tolist() == [0.0, 4.0, 0.0, 0.0, 0.0]
    assert Wc[:, 0].tolist() == [0.0, 4.5, 0.0, 0.0, 0.0] and not np.any(Wc[:, 1])
    exp = sn.Window(P, 2, 2, cfg.Lbox[:2], 4).expected([0])
    got = _run(gpu_lib, cfg, P, 4, 2, [None])
    _assert_same(got, exp, "face")
    assert got["nwrap"].tolist() == [2] and same_bits(got["D"], exp["D"])
    assert got["C"][0, :, 0].tolist() == [0.0, 2 * 4.5 ** 2, 4.5 ** 2, 4.5 ** 2, 0.0]
    assert got["D"][0, :, 0].tolist() == [0.0, 2 * 16.25, 16.25, 16.25, 0.0] and not np.any(got["D"][0, :, 1])


@pytest.mark.parametrize("dim", [1, 2, 3])
def test_counter_flow_has_no_centre_of_mass_motion(gpu_lib, dim):
    Np, Nb = 66, 3
    cfg = _dyadic(dim, Np, Nb)
    L = np.asarray(cfg.Lbox[:dim])
    sign = np.where(np.arange(Np) % 2 == 0, 1.0, -1.0)
    P = sn.drift(Np, 2 * Nb + 1, L, np.round(0.3 * L * 64.0) / 64.0, sign, np.random.default_rng(7 + dim))
    got = _run(gpu_lib, cfg, P, 2 * Nb, Nb, [None])
    assert same_bits(got["C"], np.zeros_like(got["C"])) and np.all(got["D"][0, 1:] > 0) and got["nwrap"][0] > 0
    _assert_same(got, sn.Window(P, Nb, Nb, L, 2 * Nb).expected([0]), f"counter-flow dim {dim}")


def test_exchanged_labels_leave_the_centre_of_mass(gpu_lib):
    """Particles 0 and 1, close to each other, trade labels on the upper half of the window (2^-16 grid: exact sums): the
    link sums, W and C keep their bits; the single-particle displacement D changes."""
    Np, Nb = 65, 3
    cfg = _dyadic(3, Np, Nb)
    L = np.asarray(cfg.Lbox)
    rng = np.random.default_rng(11)
    step = sn.on_grid(rng.uniform(-0.03, 0.03, (1, 2 * Nb + 1, Np, 3)) * L)
    x0 = sn.on_grid(rng.uniform(-0.5, 0.5, (1, 1, Np, 3)) * L)
    x0[0, 0, 1] = x0[0, 0, 0] + sn.on_grid(0.1 * L)
    P = sn.wrap(x0 + np.cumsum(step, axis=1), L)
    Q = P.copy()
    Q[0, Nb + 1:, [0, 1]] = P[0, Nb + 1:, [1, 0]]
    a, b = sn.Window(P, Nb, Nb, L, 2 * Nb), sn.Window(Q, Nb, Nb, L, 2 * Nb)
    assert same_bits(a.C[0], b.C[0]) and np.all(a.C[0][1:] > 0) and np.all(a.D[0][1:] != b.D[0][1:])
    ga, gb = _run(gpu_lib, cfg, P, 2 * Nb, Nb, [None]), _run(gpu_lib, cfg, Q, 2 * Nb, Nb, [None])
    _assert_same(ga, a.expected([0]), "labels kept")
    _assert_same(gb, b.expected([0]), "labels exchanged")
    assert same_bits(ga["C"], gb["C"]) and np.all(ga["D"][0, 1:] != gb["D"][0, 1:])


def test_nan_poisons_what_its_links_reach(gpu_lib):
    """A NaN in axis 1 of one particle on the LAST window slice of walker 0: only the last link has it, so U and W of axis 1
    are NaN on the last slice alone.  Every lag l >= 1 has one pair that ends there; lag 0 pairs the slice with itself.
    Axis 1 of walker 0 is NaN throughout, the other axes and walker 1 keep the bits of the clean run."""
    Np, Nb = 65, 2
    cfg = _cfg(3, Np, Nb)
    P = sn.random_walk(2, 2 * Nb + 1, Np, cfg.Lbox, np.random.default_rng(9), 0.04)
    clean = _run(gpu_lib, cfg, P, 2 * Nb, Nb, [None])
    P[0, 2 * Nb, 7, 1] = np.nan
    exp = sn.Window(P, Nb, Nb, cfg.Lbox, 2 * Nb).expected(range(2))
    assert np.all(np.isnan(exp["C"][0, :, 1])) and np.all(np.isnan(exp["D"][0, :, 1])) and np.isnan(exp["C"]).sum() == 2 * Nb + 1
    got = _run(gpu_lib, cfg, P, 2 * Nb, Nb, [None])
    _assert_same(got, exp, "NaN")
    for k in ("C", "D"):
        assert np.all(np.isnan(got[k][0, :, 1]))
        assert same_bits(got[k][0][:, [0, 2]], clean[k][0][:, [0, 2]]) and same_bits(got[k][1], clean[k][1]), k
    assert got["samples"].tolist() == [1, 1] and got["nwrap"][1] == clean["nwrap"][1]


# ---- 3. lists, launches, budgets, resets, neighbours ---------------------------------------------------------------------
def _small(dim=3, Np=65, Nb=2, W=3, seed=3):
    cfg = _cfg(dim, Np, Nb)
    return cfg, sn.random_walk(W, 2 * Nb + 1, Np, cfg.Lbox[:dim], np.random.default_rng(seed), 0.04)


def _same(a, b, ws_a=slice(None), ws_b=slice(None), f=1):
    for k in ("C", "D"):
        assert same_bits(a[k][ws_a], f * b[k][ws_b]), k
    for k in ("nwrap", "samples"):
        assert np.array_equal(a[k][ws_a], f * b[k][ws_b]), k


def test_walker_list_order_and_a_walker_listed_twice(gpu_lib):
    cfg, P = _small()
    once = _run(gpu_lib, cfg, P, 4, 2, [[0, 1, 2]])
    _assert_same(once, sn.Window(P, 2, 2, cfg.Lbox, 4).expected(range(3)), "listed")
    _same(_run(gpu_lib, cfg, P, 4, 2, [[2, 0, 1]]), once)
    _same(_run(gpu_lib, cfg, P, 4, 2, [[1], [2, 0]]), once)
    twice = _run(gpu_lib, cfg, P, 4, 2, [[0, 0, 1, 2, 2]])
    for w, f in ((0, 2), (1, 1), (2, 2)):
        _same(twice, once, w, w, f)


def test_launch_split_at_256_walkers(gpu_lib):
    """300 walkers of an Np = 3, Nb = 1 system: two launches; every walker has what a call with it alone gives."""
    W, Nb = 300, 1
    cfg = _cfg(3, 3, Nb)
    P = sn.random_walk(W, 3, 3, cfg.Lbox, np.random.default_rng(300), 0.1)
    VT, WF = gpu_lib.build_tables(cfg)
    with gpu_lib.PigsContext(cfg, VT, WF, n_walkers=W) as ctx:
        ctx.upload_all(P)
        ctx.sf_init(2, Nb)
        ctx.sf_accumulate()
        allw = ctx.sf_read(reset=True)
        for w in range(W):
            ctx.sf_accumulate([w])
        each = ctx.sf_read()
    exp = sn.Window(P, Nb, Nb, cfg.Lbox, 2).expected(range(W))
    assert exp["nwrap"].sum() > 0
    _assert_same(allw, exp, "300 walkers")
    _same(allw, each)
    assert allw["samples"].tolist() == [1] * W


def test_scratch_budget_split(gpu_lib):
    """A budget of 1 MiB holds 15 walkers of Np = 300 over nine slices (8 * 9 * 3 * 304 bytes each): 40 walkers go in three
    launches, with the bits of the one launch that the default budget gives."""
    W, Np, Nb = 40, 300, 4
    cfg = _cfg(3, Np, Nb)
    P = sn.random_walk(W, 2 * Nb + 1, Np, cfg.Lbox, np.random.default_rng(40), 0.04)
    assert (1 << 20) // (8 * 9 * 3 * 304) == 15
    VT, WF = gpu_lib.build_tables(cfg)
    with gpu_lib.PigsContext(cfg, VT, WF, n_walkers=W) as ctx:
        ctx.upload_all(P)
        ctx.sf_init(2 * Nb, Nb)
        ctx.sf_accumulate()
        whole = ctx.sf_read()
        ctx.set_tuning("sf_scratch_mib", 1)
        ctx.sf_init(2 * Nb, Nb)
        ctx.sf_accumulate()
        ctx.sf_accumulate(np.arange(W)[::-1])
        split = ctx.sf_read()
        ARG = ST["PIGS_ERR_ARG"]
        assert ctx.L.pigs_set_tuning(ctx.h, b"sf_scratch_mib", 0) == ARG and ctx.L.pigs_set_tuning(ctx.h, b"sf_scratch_mib", 2049) == ARG
    _same(split, whole, f=2)
    _assert_same(whole, sn.Window(P, Nb, Nb, cfg.Lbox, 2 * Nb).expected(range(W)), "budget")


def test_number_of_walkers_of_the_context(gpu_lib):
    cfg, P = _small()
    three = _run(gpu_lib, cfg, P, 4, 2, [None])
    alone = _run(gpu_lib, cfg, P[2:3], 4, 2, [None])
    _same(three, alone, slice(2, 3), slice(0, 1))


def test_reset_mask(gpu_lib):
    cfg, P = _small()
    VT, WF = gpu_lib.build_tables(cfg)
    with gpu_lib.PigsContext(cfg, VT, WF, n_walkers=3) as ctx:
        ctx.upload_all(P)
        ctx.sf_init(2, 1)
        ctx.sf_accumulate()
        first = ctx.sf_read(reset=[0, 1, 0])
        again = ctx.sf_read()
        ctx.sf_accumulate()
        last = ctx.sf_read(reset=True)
        zero = ctx.sf_read()
    for k in ("C", "D", "nwrap", "samples"):
        assert np.array_equal(again[k][[0, 2]], first[k][[0, 2]]) and not np.any(again[k][1]), k
        assert np.array_equal(last[k][[0, 2]], 2 * first[k][[0, 2]]) and np.array_equal(last[k][1], first[k][1]), k
        assert not np.any(zero[k]), k
    assert first["samples"].tolist() == [1, 1, 1] and np.all(first["D"][:, 1:] > 0)


def test_interleaved_with_fqs_and_lat(gpu_lib):
    """pigs_fqs_accumulate and pigs_lat_accumulate between two pigs_sf_accumulate on one context: each family keeps the
    bits it has alone."""
    import lat_numpy as ln
    cfg, P = _small()
    R = ln.grid_sites(3, 5, cfg.Lbox, cfg.Np)
    VT, WF = gpu_lib.build_tables(cfg)

    def run(sf, others):
        with gpu_lib.PigsContext(cfg, VT, WF, n_walkers=3) as ctx:
            ctx.upload_all(P)
            if sf:
                ctx.sf_init(4, 2)
            if others:
                ctx.fqs_init(2, 4, 2)
                ctx.lat_init(R, 8, 1.0, 2, 1)
            for _ in range(2):
                if sf:
                    ctx.sf_accumulate()
                if others:
                    ctx.fqs_accumulate([2, 0])
                    ctx.lat_accumulate([1])
            return (ctx.sf_read() if sf else None), ((ctx.fqs_read(), ctx.lat_read()) if others else None)

    sf_alone, _ = run(True, False)
    _, (fqs_alone, lat_alone) = run(False, True)
    sf_both, (fqs_both, lat_both) = run(True, True)
    _same(sf_both, sf_alone)
    assert sf_both["samples"].tolist() == [2, 2, 2]
    for a, b in ((fqs_alone, fqs_both), (lat_alone, lat_both)):
        for k in a:
            assert same_bits(a[k], b[k]) if a[k].dtype == np.float64 else np.array_equal(a[k], b[k]), k


# ---- 4. refusals ------------------------------------------------------------------------------------------------------
def test_status_codes(gpu_lib):
    Nb = 3
    ARG, OK, UNS = ST["PIGS_ERR_ARG"], ST["PIGS_OK"], ST["PIGS_ERR_UNSUPPORTED"]
    cfg = _cfg(2, 30, Nb)
    VT, WF = gpu_lib.build_tables(cfg)
    with gpu_lib.PigsContext(cfg, VT, WF, n_walkers=2) as ctx:
        init = lambda Ntau, window: ctx.L.pigs_sf_init(ctx.h, Ntau, window)
        assert ctx.L.pigs_sf_accumulate(ctx.h, 1, None) == ARG              # before init
        with pytest.raises(gpu_lib.PigsError):
            ctx.sf_read()
        d, l = np.zeros(8), np.zeros(2, np.int64)
        dp, lp = d.ctypes.data_as(C.POINTER(C.c_double)), l.ctypes.data_as(C.POINTER(C.c_int64))
        assert ctx.L.pigs_sf_read(ctx.h, dp, dp, lp, lp, None) == ARG
        for args in ((0, -1), (0, Nb + 1), (-1, 1), (3, 1), (1, 0), (2 * Nb + 1, Nb)):
            assert init(*args) == ARG, args
            assert ctx.L.pigs_sf_accumulate(ctx.h, 1, None) == ARG
        assert init(0, 0) == OK and init(2 * Nb, Nb) == OK and init(0, Nb) == OK
        assert ctx.L.pigs_sf_accumulate(ctx.h, -1, None) == ARG
        assert ctx.L.pigs_sf_accumulate(ctx.h, 1, np.array([2], np.int32).ctypes.data_as(_ip)) == ARG
        assert ctx.L.pigs_sf_accumulate(ctx.h, 1, np.array([-1], np.int32).ctypes.data_as(_ip)) == ARG
        assert ctx.L.pigs_sf_accumulate(ctx.h, 0, None) == OK
        ctx.sync()
    # more than 3072 lags.  (Accumulators beyond 2 GiB need 14 564 walkers of 3 072 lags in 3D, whose worldlines alone take
    # 8.6 GB: that refusal is not exercised here.)
    long_ = SystemConfig(dim=2, Np=2, Nb=1600, density=0.25)
    VT, WF = gpu_lib.build_tables(long_)
    with gpu_lib.PigsContext(long_, VT, WF, n_walkers=1) as ctx:
        assert ctx.L.pigs_sf_init(ctx.h, 3072, 1600) == ARG and ctx.L.pigs_sf_init(ctx.h, 3071, 1600) == OK
        ctx.sync()
    tcfg = SystemConfig(dim=2, Np=6, Nb=2, trap=True, a_ho=[1.0, 1.3], Nmax=2000, Rm=1.2, dt=0.01)
    VT, WF = gpu_lib.build_tables(tcfg)
    with gpu_lib.PigsContext(tcfg, VT, WF, n_walkers=1) as ctx:
        assert ctx.L.pigs_sf_init(ctx.h, 0, 0) == UNS
        assert ctx.L.pigs_sf_accumulate(ctx.h, 1, None) == ARG
        ctx.sync()


# ---- 5. the front end ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def exe(gpu_lib):
    import subprocess
    host = os.path.join(ROOT, "pathintegralgroundstate_amd", "host")
    subprocess.check_call(["make", "-s", "-C", host])
    return os.path.join(host, "pigs_vpi")


def _rundir(tmp_path, name, run):
    import shutil
    from test_gpu_front_end_blocks import RUNS
    d = str(tmp_path / name)
    os.makedirs(d)
    if os.path.exists(os.path.join(RUNS, run, "config_ini.in")):
        shutil.copy(os.path.join(RUNS, run, "config_ini.in"), d)
    return d


@pytest.mark.parametrize("run", ["he4_cworm0", "he4_crystal"])
def test_front_end_two_blocks_three_steps(gpu_lib, oracle, exe, tmp_path, run):
    """he4_cworm0 (2D, nine particles, no worm sector) and he4_crystal (3D, started on the sites of config_ini.in, worm
    sector on), 2 blocks x 3 steps, two walkers, superfluid = T over the lags 0..4 of a window of 2: every file of the run
    without the key byte for byte, with either sampler; the two new files of every walker against a replay of the run's
    chains through PigsContext.sf_* and normalize_sf; two shards on one GPU give one shard's per-walker files byte for
    byte."""
    from test_gpu_front_end_blocks import RUNS, _input, _run as run_vpi, replay
    from test_sf_host import check_files
    W, Nblock, Nstep, window, Ntau = 2, 2, 3, 2, 4
    txt, cfg = _input(run, Nblock, Nstep)
    start = None
    if run == "he4_crystal":
        ini = open(os.path.join(RUNS, run, "config_ini.in")).read().split("\n")
        cfg = SystemConfig.from_namelists(txt, Np=int(ini[0]), density=float(ini[2]), Lbox=[float(x) for x in ini[1].split()])
        start = np.array([[float(x) for x in l.split()] for l in ini[3:3 + int(ini[0])]])
    assert not cfg.trap and cfg.Nb >= window
    key = f", superfluid = T, sf_ntau = {Ntau}, sf_window = {window}"
    rep = replay(gpu_lib, oracle, cfg, W, Nblock, Nstep, start=start)
    VT, WF = gpu_lib.build_tables(cfg)
    blocks = []
    with gpu_lib.PigsContext(cfg, VT, WF, n_walkers=W) as ctx:
        ctx.sf_init(Ntau, window)
        for b in range(Nblock):
            for t in range(b * Nstep, (b + 1) * Nstep):
                ctx.upload_all(rep["snaps"][t])
                wl = np.nonzero(rep["diag"][t])[0]
                if len(wl):
                    ctx.sf_accumulate(wl)
            blocks.append(ctx.sf_read(reset=True))
    counted = np.stack([b["samples"] > 0 for b in blocks], axis=1)           # [W, Nblock]
    assert counted.any() and max(float(b["D"][:, 1:].max()) for b in blocks) > 0
    first = None
    for ds in ("T", "F"):
        plain, on = _rundir(tmp_path, "plain" + ds, run), _rundir(tmp_path, "on" + ds, run)
        run_vpi(exe, txt + f"&gpu\n n_walkers = {W}, device_sampler = {ds}\n/\n", plain)
        out = run_vpi(exe, txt + f"&gpu\n n_walkers = {W}, device_sampler = {ds}{key}\n/\n", on)
        assert "Superfluid fraction" in out
        old = sorted(os.listdir(plain))
        new = sorted(set(os.listdir(on)) - set(old))
        assert sorted(f for f in new if ".w" not in f) == ["msdu_vpi.out", "rhos_vpi.out"], new
        assert len(new) == 2 + 2 * W, new
        for f in old:
            if f not in ("stdout.txt", "vpi.in"):
                assert open(os.path.join(plain, f), "rb").read() == open(os.path.join(on, f), "rb").read(), f
        final = np.fromfile(os.path.join(on, "worldlines_final.bin")).reshape(rep["final"].shape)
        assert np.array_equal(final, rep["final"])
        names = sorted(f for f in new if re.fullmatch(r"rhos_vpi\.w\d+\.out", f))
        assert len(names) == W
        for w, fr in enumerate(names):
            bs = [b for b in range(Nblock) if counted[w, b]]
            if not bs:
                continue
            mine = [normalize_sf({k: (v[w] if k != "window" else v) for k, v in blocks[b].items()}, cfg.Np, cfg.dt) for b in bs]
            # (the error of two blocks is a difference of two nearly equal moments printed to ten digits)
            check_files(os.path.join(on, fr), os.path.join(on, fr.replace("rhos_", "msdu_")), mine, cfg.dim, Ntau, cfg.dt)
        if first is None:
            first = on
        else:                                                           # the two samplers give the same files
            for f in new:
                assert open(os.path.join(first, f), "rb").read() == open(os.path.join(on, f), "rb").read(), f
    two = _rundir(tmp_path, "two", run)
    run_vpi(exe, txt + f"&gpu\n n_walkers = {W}, device_sampler = T, device = 0, n_gpus = 2, same_device = T{key}\n/\n", two)
    for f in sorted(os.listdir(first)):
        if ".w" in f and f.endswith(".out"):
            assert open(os.path.join(first, f), "rb").read() == open(os.path.join(two, f), "rb").read(), f


@pytest.mark.parametrize("keys,word", [("sf_ntau = 5, sf_window = 2", "sf_ntau"), ("sf_ntau = 1000", "sf_window")])
def test_front_end_refuses_bad_lags_before_any_gpu_work(gpu_lib, exe, tmp_path, keys, word):
    import subprocess
    from test_gpu_front_end_blocks import _input
    txt, _ = _input("he4_cworm0", 1, 1)
    wd = _rundir(tmp_path, "bad", "he4_cworm0")
    with open(os.path.join(wd, "vpi.in"), "w") as f:
        f.write(txt + f"&gpu\n superfluid = T, {keys}\n/\n")
    with open(os.path.join(wd, "vpi.in")) as fin:
        r = subprocess.run([exe], stdin=fin, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, cwd=wd, timeout=120)
    out = r.stdout.decode(errors="replace")
    assert r.returncode == 2 and "superfluid" in out and word in out, out[-2000:]
    assert not os.path.exists(os.path.join(wd, "e_vpi.out"))


def test_front_end_refuses_a_trapped_run(gpu_lib, exe, tmp_path):
    import subprocess
    from test_gpu_front_end_blocks import _input
    txt, cfg = _input("trap2d_bis_cworm0", 1, 1)
    assert cfg.trap
    wd = _rundir(tmp_path, "trap", "trap2d_bis_cworm0")
    with open(os.path.join(wd, "vpi.in"), "w") as f:
        f.write(txt + "&gpu\n superfluid = T\n/\n")
    with open(os.path.join(wd, "vpi.in")) as fin:
        r = subprocess.run([exe], stdin=fin, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, cwd=wd, timeout=120)
    out = r.stdout.decode(errors="replace")
    assert r.returncode == 2 and "superfluid" in out and "periodic" in out, out[-2000:]
    assert not os.path.exists(os.path.join(wd, "e_vpi.out"))
