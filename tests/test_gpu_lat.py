"""The lattice sums of a crystal on the MI355X (pigs_lat_*, pigs_lat.hip), through the C ABI.

The expected sums come from the numpy restatement in tests/lat_numpy.py (the same IEEE operations per term; pinned to a
literal loop and to closed forms by tests/test_lat_numpy_host.py).  Every integer array must be EQUAL.  The bound on mom
per element is 1e-12 * Sum|terms| from the numpy side, the project's bound for a fixed-order sum (tests/test_gpu_atm.py);
every term is a square, so Sum|terms| is the sum itself.  Where an element holds one non-zero term it must have the
restatement's bits.  No comparison masks or skips elements.  The inputs are jittered lattices in a box of unequal sides:
particle i sits near site i (mod the sites), so nsite = Np - 1 doubles one site and nsite = Np + 1 leaves one empty.
Such a lattice of cell centres never reaches the fold of the winner's displacement, the tile boundary of the site loop,
the class "three or more", the assigned count below Np with cm = 1 or the ends of the axis histograms: section 2b builds
those by hand and asserts on the numpy side that each case reaches its branch.

Largest |got - want| / bound seen on the MI355X: see DESIGN.md (the lattice section)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import lat_numpy as ln
from conftest import ROOT
from helpers import same_bits
from pathintegralgroundstate_amd import SystemConfig
from pathintegralgroundstate_amd.profiles import nearest_neighbour_distance

pytestmark = pytest.mark.gpu
DENSITY = {2: 0.25, 3: 0.365}
_dp = C.POINTER(C.c_double)


def _header():
    return open(os.path.join(ROOT, "include", "pigs_hip.h")).read()


ST = {k: int(v) for k, v in re.findall(r"^\s*(PIGS_\w+)\s*=\s*(-?\d+)", _header(), flags=re.M)}
assert ST["PIGS_OK"] == 0 and len({ST["PIGS_ERR_ARG"], ST["PIGS_ERR_HIP"], ST["PIGS_ERR_UNSUPPORTED"]}) == 3


def _cfg(dim, Np, Nb):
    """A box of unequal sides at the family's density."""
    L = (Np / DENSITY[dim]) ** (1.0 / dim)
    return SystemConfig(dim=dim, Np=Np, Nb=Nb, density=DENSITY[dim],
                        Lbox=[0.8 * L, 1.25 * L] if dim == 2 else [0.8 * L, 1.25 * L, L])


def _lattice(cfg, nsite):
    """(sites [nsite, dim], the smallest spacing of the grid they are taken from)"""
    dim = cfg.dim
    n = int(np.ceil((cfg.Np + 1) ** (1.0 / dim) - 1e-9))
    return ln.grid_sites(dim, n, cfg.Lbox, nsite), min(cfg.Lbox[:dim]) / n


def _assert_same(got, exp, what):
    for k in ln.INT_KEYS:
        assert got[k].dtype == np.int64 and got[k].shape == exp[k].shape, (what, k)
        assert np.array_equal(got[k], exp[k]), (what, k, int(np.abs(got[k] - exp[k]).sum()))
    assert got["mom"].shape == exp["mom"].shape and got["mom"].dtype == np.float64
    assert np.all(np.isfinite(exp["mom"])) and np.all(np.isfinite(got["mom"])), what
    bound = 1e-12 * np.abs(exp["mom"])
    err = np.abs(got["mom"] - exp["mom"])
    with np.errstate(all="ignore"):
        worst = float(np.max(np.where(err == 0, 0.0, err / bound)))
    print(f"{what}: max |got-want|/bound = {worst:.3e} over {err.size} elements")
    assert np.all(err <= bound), (what, worst)


def _run(gpu_lib, cfg, paths, sites, nbin, rmax, window, cm, lists):
    VT, WF = gpu_lib.build_tables(cfg)
    with gpu_lib.PigsContext(cfg, VT, WF, n_walkers=paths.shape[0]) as ctx:
        ctx.upload_all(paths)
        ctx.lat_init(sites, nbin, rmax, window, cm)
        for wl in lists:
            ctx.lat_accumulate(wl)
        return ctx.lat_read()


# ---- 1. against the numpy restatement -----------------------------------------------------------------------------------
@pytest.mark.parametrize("dn", [0, 1, -1])
@pytest.mark.parametrize("Np", [3, 64, 65, 257, 300])
@pytest.mark.parametrize("dim", [2, 3])
def test_matches_numpy(gpu_lib, dim, Np, dn):
    """nsite = Np + dn; windows 0 and Nb and cm 0 and 1 on one context (lat_init again resizes and zeroes).  rmax is 0.2
    spacings against a jitter of +-0.2 per axis: some |v| fall beyond the radial histogram."""
    Nb, W, nbin = 3, 2, 12
    cfg = _cfg(dim, Np, Nb)
    R, a = _lattice(cfg, Np + dn)
    P = ln.jittered(R, W, 2 * Nb + 1, Np, cfg.Lbox, np.random.default_rng(100 * dim + Np + dn), 0.2 * a)
    rmax = 0.2 * a
    VT, WF = gpu_lib.build_tables(cfg)
    with gpu_lib.PigsContext(cfg, VT, WF, n_walkers=W) as ctx:
        ctx.upload_all(P)
        for window in (0, Nb):
            for cm in (0, 1):
                exp = ln.Window(P, Nb, window, cfg.Lbox, R, nbin, rmax, cm).expected(range(W))
                ctx.lat_init(R, nbin, rmax, window, cm)
                ctx.lat_accumulate()
                got = ctx.lat_read()
                _assert_same(got, exp, f"dim {dim} Np {Np} nsite {Np + dn} window {window} cm {cm}")
                assert np.all(exp["nlost"] == 0) and np.all(exp["nassigned"] == Np)
                assert np.all(exp["occ"][..., 0] == max(dn, 0)) and np.all(exp["occ"][..., 2] == max(-dn, 0))
                assert Np < 64 or 0 < exp["hr"].sum() < exp["nassigned"].sum()      # some |v| inside the histogram, some beyond


def test_large_system(gpu_lib):
    """Np = nsite = 1077 in 3D: five rounds of particles over five tiles of sites."""
    Np, Nb = 1077, 1
    cfg = _cfg(3, Np, Nb)
    R, a = _lattice(cfg, Np)
    P = ln.jittered(R, 1, 3, Np, cfg.Lbox, np.random.default_rng(1077), 0.2 * a)
    exp = ln.Window(P, Nb, 0, cfg.Lbox, R, 20, 0.4 * a, 1).expected([0])
    got = _run(gpu_lib, cfg, P, R, 20, 0.4 * a, 0, 1, [None])
    _assert_same(got, exp, "Np 1077")
    assert exp["occ"][0, 0].tolist() == [0, Np, 0, 0]


@pytest.mark.parametrize("dim", [2, 3])
def test_exchanged_labels_along_tau(gpu_lib, dim):
    """Particles 0 and 1 trade places on the upper half of the window: two hops per link crossing, two across the window."""
    Np, Nb = 65, 2
    cfg = _cfg(dim, Np, Nb)
    R, a = _lattice(cfg, Np)
    P = ln.jittered(R, 2, 2 * Nb + 1, Np, cfg.Lbox, np.random.default_rng(5 + dim), 0.1 * a)
    P[1, Nb + 1:, [0, 1]] = P[1, Nb + 1:, [1, 0]]
    exp = ln.Window(P, Nb, Nb, cfg.Lbox, R, 8, 0.5 * a, 1).expected(range(2))
    got = _run(gpu_lib, cfg, P, R, 8, 0.5 * a, Nb, 1, [None])
    _assert_same(got, exp, f"exchange dim {dim}")
    assert got["hop1"].tolist() == [0, 2] and got["hopw"].tolist() == [0, 2]


# ---- 2. edges: bit for bit ---------------------------------------------------------------------------------------------
def _one_moving(dim, x, nbin, rmax, x0=-1.0):
    """Three particles and three sites in a wide box: particles 1 and 2 sit on sites 1 and 2, particle 0 at x; site 0 at
    (x0, 0, ..)."""
    cfg = SystemConfig(dim=dim, Np=3, Nb=1, density=3.0 / 40.0 ** dim)
    R = np.zeros((3, dim))
    R[0, 0], R[1, 0], R[2, 1] = x0, 1.0, 9.0
    X = R.copy()
    X[0] = x
    P = np.broadcast_to(X, (1, 3, 3, dim)).copy()
    return cfg, R, P


@pytest.mark.parametrize("dim", [2, 3])
def test_tie_takes_the_lower_site(gpu_lib, dim):
    """Particle 0 at the origin, sites 0 and 1 at x = -1 and +1: r2 = 1 for both, site 0 wins, u = (+1, 0, ..); site 1
    then holds its own particle only."""
    x = np.zeros(dim)
    cfg, R, P = _one_moving(dim, x, 4, 2.0)
    exp = ln.Window(P, 1, 1, cfg.Lbox, R, 4, 2.0, 0).expected([0])
    got = _run(gpu_lib, cfg, P, R, 4, 2.0, 1, 0, [None])
    _assert_same(got, exp, "tie")
    assert same_bits(got["mom"], exp["mom"]) and np.all(got["mom"][0, :, 0] == 1.0)
    assert got["occ"][0].tolist() == [[0, 3, 0, 0]] * 3 and got["hx"][0, 0, 6] == 3        # v_x = +1 of [-2, 2) in 8 bins


@pytest.mark.parametrize("dim", [2, 3])
@pytest.mark.parametrize("below", [True, False])
def test_bin_edge_one_ulp(gpu_lib, dim, below):
    """|v| one ulp below rmax and at rmax: the radial bin is decided in double before the conversion."""
    rmax, nbin = 0.7, 7
    d = np.nextafter(rmax, 0.0) if below else rmax
    x = np.zeros(dim)
    x[0] = -1.0 + d                                                     # u = d exactly? whatever it is, numpy has its bits
    cfg, R, P = _one_moving(dim, x, nbin, rmax)
    exp = ln.Window(P, 1, 0, cfg.Lbox, R, nbin, rmax, 0).expected([0])
    got = _run(gpu_lib, cfg, P, R, nbin, rmax, 0, 0, [None])
    _assert_same(got, exp, f"edge below={below}")
    assert same_bits(got["mom"], exp["mom"])
    assert int(got["hr"].sum()) in (2, 3) and np.array_equal(got["hr"], exp["hr"]) and np.array_equal(got["hx"], exp["hx"])


def test_nan_coordinate_is_lost(gpu_lib):
    """A NaN coordinate on one slice: that particle is lost there, adds to nothing, and every other count stays."""
    Np, Nb = 65, 1
    cfg = _cfg(3, Np, Nb)
    R, a = _lattice(cfg, Np)
    P = ln.jittered(R, 1, 3, Np, cfg.Lbox, np.random.default_rng(9), 0.1 * a)
    clean = ln.Window(P, Nb, Nb, cfg.Lbox, R, 8, 0.5 * a, 0).expected([0])
    P[0, Nb, 7, 1] = np.nan
    exp = ln.Window(P, Nb, Nb, cfg.Lbox, R, 8, 0.5 * a, 0).expected([0])
    got = _run(gpu_lib, cfg, P, R, 8, 0.5 * a, Nb, 0, [None])
    _assert_same(got, exp, "NaN")
    assert got["nlost"].tolist() == [1] and got["nassigned"].tolist() == [[Np, Np - 1, Np]]
    assert got["occ"][0, 1].tolist() == [1, Np - 1, 0, 0] and np.array_equal(got["occ"][0, ::2], clean["occ"][0, ::2])
    assert got["hop1"].tolist() == [0] and int(got["hr"].sum()) == int(clean["hr"].sum()) - 1


# ---- 2b. the branches that a jittered lattice of cell centres never takes -------------------------------------------------
# Every condition that makes a case meaningful is asserted on the numpy side, so that a case which no longer reaches its
# branch fails rather than passes.
_tile = re.search(r"constexpr\s+int\s+kLatTile\s*=\s*(\d+)\s*;", open(os.path.join(
    ROOT, "pathintegralgroundstate_amd", "csrc", "pigs_kernels.h")).read())
assert _tile, "kLatTile is not in csrc/pigs_kernels.h"
TILE = int(_tile.group(1))
ROUND = 256                     # kLatThreads: the classification loop takes the sites in rounds of 256


def _face_lattice(dim):
    """8 x 8 or 4 x 4 x 4 sites ON the faces of a box of unequal sides: grid_sites' grid shifted by half a cell, so the
    first row of every axis sits at -L_k/2; particles jittered by 0.3 of the smallest spacing and wrapped."""
    n = 8 if dim == 2 else 4
    cfg = _cfg(dim, 64, 1)
    L = np.asarray(cfg.Lbox[:dim])
    idx = np.stack(np.unravel_index(np.arange(n ** dim), (n,) * dim), axis=1).astype(np.float64)
    R = idx * (L / n) - 0.5 * L
    assert R.shape == (64, dim) and np.all(R.min(axis=0) == -0.5 * L) and np.all(R.max(axis=0) < 0.5 * L)
    P = ln.jittered(R, 1, 3, 64, cfg.Lbox, np.random.default_rng(40 + dim), 0.3 * min(L) / n)
    return cfg, R, P


@pytest.mark.parametrize("dim", [2, 3])
def test_winner_across_a_periodic_face(gpu_lib, dim):
    """Sites on the box faces: a particle jittered below -L_k/2 is wrapped to the far side of the box, so its own site wins
    only through the fold, and the winner's u is the folded difference.  Window 1, cm 0 and 1."""
    cfg, R, P = _face_lattice(dim)
    L = np.asarray(cfg.Lbox[:dim])
    for a in range(3):
        site, u = ln.assign(P[0, a], R, cfg.Lbox)
        raw = P[0, a] - R[site]
        assert np.array_equal(site, np.arange(64))
        assert np.all((np.abs(raw) > 0.5 * L).sum(axis=0) >= 1), "no winner across a face on some axis"
        assert np.all(np.abs(u) < 0.5 * L) and np.any(u != raw)
    rmax = 0.35 * min(L) / (8 if dim == 2 else 4)
    VT, WF = gpu_lib.build_tables(cfg)
    with gpu_lib.PigsContext(cfg, VT, WF, n_walkers=1) as ctx:
        ctx.upload_all(P)
        for cm in (0, 1):
            exp = ln.Window(P, 1, 1, cfg.Lbox, R, 8, rmax, cm).expected([0])
            assert np.all(exp["nassigned"] == 64) and np.all(exp["occ"] == [0, 64, 0, 0]) and exp["nlost"].tolist() == [0]
            ctx.lat_init(R, 8, rmax, 1, cm)
            ctx.lat_accumulate()
            _assert_same(ctx.lat_read(), exp, f"face dim {dim} cm {cm}")


def _line_case(dim, nsite):
    """Sites on a line along x, 0.25 apart (every difference, square and sum is exact), in a box of 256 x 16 (x 16) that
    holds them without a fold.  One slice.  Particles ON sites 0, TILE-1, TILE, nsite-1 and 2 TILE-1 (the first and the last
    column of a tile, on either side of a tile boundary), one at the exact midpoint of sites TILE-1 and TILE, three on
    site ROUND+44 and four on site ROUND+144 -- whichever of these sites exist at this nsite."""
    x = lambda s: np.array([0.25 * s - 64.0] + [0.0] * (dim - 1))
    R = np.stack([x(s) for s in range(nsite)])
    on = sorted({s for s in (0, TILE - 1, TILE, nsite - 1, 2 * TILE - 1) if 0 <= s < nsite})
    X = [x(s) for s in on]
    tie = TILE < nsite
    if tie:
        X.append(0.5 * (x(TILE - 1) + x(TILE)))
    loads = {s: n for s, n in ((ROUND + 44, 3), (ROUND + 144, 4)) if s < nsite and s not in on}
    for s, n in loads.items():
        X += [x(s)] * n
    X = np.stack(X)
    Np = X.shape[0]
    Lbox = [256.0, 16.0] if dim == 2 else [256.0, 16.0, 16.0]
    cfg = SystemConfig(dim=dim, Np=Np, Nb=1, density=Np / float(np.prod(Lbox)), Lbox=Lbox)
    P = np.broadcast_to(X, (1, 3, Np, dim)).copy()
    return cfg, R, P, on, tie, loads


@pytest.mark.parametrize("dim", [2, 3])
@pytest.mark.parametrize("dn", ["T-1", "T", "T+1", "2T+1"])
def test_tile_boundary_of_the_site_loop(gpu_lib, dim, dn):
    """nsite = kLatTile - 1, kLatTile, kLatTile + 1 and 2 kLatTile + 1: winners in the first and the last column of a tile;
    a tie between the last site of one tile and the first of the next, where `best` must carry over with a strict `<`;
    sites with three and with four particles in the classifier's second round.  cm = 0 and exact arithmetic: bit for bit."""
    nsite = {"T-1": TILE - 1, "T": TILE, "T+1": TILE + 1, "2T+1": 2 * TILE + 1}[dn]
    cfg, R, P, on, tie, loads = _line_case(dim, nsite)
    X = P[0, 1]
    site, u = ln.assign(X, R, cfg.Lbox)
    assert site[:len(on)].tolist() == on and not np.any(u[:len(on)]) and {0, nsite - 1, min(TILE - 1, nsite - 1)} <= set(on)
    if tie:
        i = len(on)
        d = ln.fold(X[i] - R[[TILE - 1, TILE]], cfg.Lbox)
        r2 = ln.r2_of(d)
        assert same_bits(r2[0], r2[1]) and r2[0] == 0.125 ** 2 and site[i] == TILE - 1 and u[i, 0] == 0.125
    assert (nsite > TILE) == tie and (nsite == 2 * TILE + 1) == (len(loads) == 2)
    exp = ln.Window(P, 1, 0, cfg.Lbox, R, 8, 1.0, 0).expected([0])
    per = np.bincount(site, minlength=nsite)
    if loads:                                                           # both flavours of "three or more", beyond site 255
        assert min(loads) >= ROUND and sorted(per[per >= 3].tolist()) == [3, 4] and np.all(np.flatnonzero(per >= 3) >= ROUND)
        assert exp["occ"][0, 0, 3] == 2 and per[2 * TILE - 1] == 1 and per[nsite - 1] == 1
    assert exp["occ"][0, 0].tolist() == [int((per == q).sum()) for q in (0, 1, 2)] + [int((per >= 3).sum())]
    got = _run(gpu_lib, cfg, P, R, 8, 1.0, 0, 0, [None])
    _assert_same(got, exp, f"tile dim {dim} nsite {nsite}")
    assert same_bits(got["mom"], exp["mom"])
    assert got["mom"][0, 0, 0] == (0.125 ** 2 if tie else 0.0)


@pytest.mark.parametrize("Np,nsite", [(1077, 5), (5, 1077)])
def test_many_particles_on_few_sites_and_few_on_many(gpu_lib, Np, nsite):
    """Np = 1077 on nsite = 5 (five rounds of particles, one short tile, every site holds 215 or more) and Np = 5 on
    nsite = 1077 (five tiles and five rounds of the classifier, 1072 vacant sites), 3D, one slice."""
    cfg = _cfg(3, Np, 1)
    R = ln.grid_sites(3, 11, cfg.Lbox, nsite)
    a = min(cfg.Lbox) / 11
    P = ln.jittered(R, 1, 3, Np, cfg.Lbox, np.random.default_rng(Np), 0.2 * a)
    exp = ln.Window(P, 1, 0, cfg.Lbox, R, 20, 0.4 * a, 1).expected([0])
    assert exp["occ"][0, 0].tolist() == ([0, 0, 0, 5] if nsite == 5 else [1072, 5, 0, 0]) and exp["nassigned"][0, 0] == Np
    got = _run(gpu_lib, cfg, P, R, 20, 0.4 * a, 0, 1, [None])
    _assert_same(got, exp, f"Np {Np} nsite {nsite}")


@pytest.mark.parametrize("dim", [2, 3])
def test_occupancy_ladder(gpu_lib, dim):
    """Ten particles on six sites with 0, 1, 2, 3, 4 and 0 particles: two vacant, one single, one double, two of class
    "three or more"."""
    cfg = _cfg(dim, 10, 1)
    R, a = _lattice(cfg, 6)
    home = np.array([1, 2, 2, 3, 3, 3, 4, 4, 4, 4])
    L = np.asarray(cfg.Lbox[:dim])
    P = R[home][None, None] + np.random.default_rng(6 + dim).uniform(-0.2 * a, 0.2 * a, (1, 3, 10, dim))
    P = P - L * np.floor((P + 0.5 * L) / L)
    exp = ln.Window(P, 1, 1, cfg.Lbox, R, 8, 0.4 * a, 1).expected([0])
    assert np.all(exp["occ"][0] == [2, 1, 1, 2]) and np.all(exp["nassigned"] == 10)
    got = _run(gpu_lib, cfg, P, R, 8, 0.4 * a, 1, 1, [None])
    _assert_same(got, exp, f"ladder dim {dim}")
    assert got["occ"][0].tolist() == [[2, 1, 1, 2]] * 3


def _lost_base():
    Np, Nb = 65, 2
    cfg = _cfg(3, Np, Nb)
    R, a = _lattice(cfg, Np)
    return cfg, R, a, ln.jittered(R, 1, 2 * Nb + 1, Np, cfg.Lbox, np.random.default_rng(65), 0.1 * a)


@pytest.mark.parametrize("how", ["nan", "inf"])
def test_lost_particles_and_the_centre_of_mass(gpu_lib, how):
    """cm = 1 with lost particles on the middle slice (one NaN coordinate; three particles with a +inf coordinate): the
    centre of mass divides by the ASSIGNED particles.  Dividing by Np would move mom of that slice by far more than its
    bound, which is asserted first."""
    cfg, R, a, P = _lost_base()
    Np, Nb = cfg.Np, cfg.Nb
    if how == "nan":
        P[0, Nb, 7, 1] = np.nan
    else:
        P[0, Nb, [3, 30, 64], [0, 2, 1]] = np.inf
    nl = 1 if how == "nan" else 3
    exp = ln.Window(P, Nb, Nb, cfg.Lbox, R, 8, 0.5 * a, 1).expected([0])
    site, u = ln.assign(P[0, Nb], R, cfg.Lbox)
    ok = site >= 0
    tot = np.array([np.cumsum(np.concatenate(([0.0], u[:, k])))[-1] for k in range(3)])
    m2 = lambda c: float(ln.r2_of((u - c)[ok]).sum())
    assert int(ok.sum()) == Np - nl and same_bits(m2(tot / float(Np - nl)), exp["mom"][0, Nb, 0])
    assert abs(m2(tot / float(Np)) - m2(tot / float(Np - nl))) > 1e3 * 1e-12 * exp["mom"][0, Nb, 0]
    got = _run(gpu_lib, cfg, P, R, 8, 0.5 * a, Nb, 1, [None])
    _assert_same(got, exp, f"lost ({how}) with cm")
    assert got["nlost"].tolist() == [nl] and got["nassigned"][0].tolist() == [Np, Np, Np - nl, Np, Np]
    assert got["occ"][0, Nb].tolist() == [nl, Np - nl, 0, 0]


def test_a_slice_with_every_particle_lost(gpu_lib):
    """Every particle of the middle slice has a NaN coordinate: nothing is assigned there, the division of the centre of
    mass is not taken, mom of the slice stays exactly 0.0 and every site is vacant; the other slices keep the bits of the
    clean run."""
    cfg, R, a, P = _lost_base()
    Np, Nb = cfg.Np, cfg.Nb
    clean = _run(gpu_lib, cfg, P, R, 8, 0.5 * a, Nb, 1, [None])
    P[0, Nb, :, 2] = np.nan
    exp = ln.Window(P, Nb, Nb, cfg.Lbox, R, 8, 0.5 * a, 1).expected([0])
    assert exp["nassigned"][0].tolist() == [Np, Np, 0, Np, Np] and not np.any(exp["mom"][0, Nb])
    got = _run(gpu_lib, cfg, P, R, 8, 0.5 * a, Nb, 1, [None])
    _assert_same(got, exp, "a slice lost")
    others = [0, 1, 3, 4]
    assert got["nassigned"][0, Nb] == 0 and got["nlost"].tolist() == [Np] and got["occ"][0, Nb].tolist() == [Np, 0, 0, 0]
    assert same_bits(got["mom"][0, Nb], np.zeros(5)) and same_bits(got["mom"][0, others], clean["mom"][0, others])
    assert np.array_equal(got["occ"][0, others], clean["occ"][0, others]) and got["hop1"].tolist() == [0]
    assert np.array_equal(got["nassigned"][0, others], clean["nassigned"][0, others]) and got["hopw"].tolist() == [0]


@pytest.mark.parametrize("dim", [2, 3])
@pytest.mark.parametrize("where", ["-rmax", "below -rmax", "+rmax", "below +rmax"])
def test_axis_histogram_edges(gpu_lib, dim, where):
    """v_x of particle 0 at the two ends of [-rmax, rmax), rmax = 0.5 in 2 x 4 bins of 0.125 (the division is exact):
    -rmax is t = 0.0, the first bin; one ulp below it is out; +rmax is t = 2 nbin, out; one ulp below +rmax is wherever
    (v + rmax) / rbin rounds to in double, which is written out here.  Site 0 sits at x = -0.25, so that x - R is exact."""
    rmax, nbin = 0.5, 4
    v = {"-rmax": -rmax, "below -rmax": np.nextafter(-rmax, -1.0), "+rmax": rmax, "below +rmax": np.nextafter(rmax, 0.0)}[where]
    x = np.zeros(dim)
    x[0] = -0.25 + v
    cfg, R, P = _one_moving(dim, x, nbin, rmax, x0=-0.25)
    site, u = ln.assign(P[0, 1], R, cfg.Lbox)
    assert site.tolist() == [0, 1, 2] and same_bits(u[0, 0], v) and not np.any(u[1:]) and not np.any(u[0, 1:])
    t = (float(v) + rmax) / (rmax / float(nbin))
    inside = 0.0 <= t < float(2 * nbin)
    assert inside == {"-rmax": True, "below -rmax": False, "+rmax": False}.get(where, inside)
    assert where != "-rmax" or t == 0.0
    exp = ln.Window(P, 1, 0, cfg.Lbox, R, nbin, rmax, 0).expected([0])
    want = np.zeros(2 * nbin, np.int64)
    want[nbin] = 2                                                      # particles 1 and 2: v = 0
    if inside:
        want[int(t)] += 1
    assert exp["hx"][0, 0].tolist() == want.tolist() and np.all(exp["hx"][0, 1:, nbin] == 3)
    got = _run(gpu_lib, cfg, P, R, nbin, rmax, 0, 0, [None])
    _assert_same(got, exp, f"axis edge {where} dim {dim}")
    assert same_bits(got["mom"], exp["mom"]) and got["hx"][0, 0].tolist() == want.tolist()


@pytest.mark.parametrize("dim", [2, 3])
def test_hop_patterns(gpu_lib, dim):
    """Five slices.  Particle 5 goes A B A A A: two link hops, none across the window.  Particle 20 goes A A lost B B: no
    link hop (a lost end drops the comparison), one across the window.  Particle 40 is lost on the first slice, sits on A
    on the second and on C from the third on: one link hop, none across the window."""
    Np, Nb = 65, 2
    cfg = _cfg(dim, Np, Nb)
    R, a = _lattice(cfg, Np)
    P = ln.jittered(R, 1, 5, Np, cfg.Lbox, np.random.default_rng(50 + dim), 0.1 * a)
    quiet = ln.Window(P, Nb, Nb, cfg.Lbox, R, 8, 0.5 * a, 1).expected([0])
    assert quiet["hop1"].tolist() == [0] and quiet["hopw"].tolist() == [0]
    P[0, 1, 5] = P[0, 1, 6]
    P[0, 2, 20, 0] = np.nan
    P[0, 3:, 20] = P[0, 3:, 21]
    P[0, 0, 40, dim - 1] = np.nan
    P[0, 2:, 40] = P[0, 2:, 41]
    w = ln.Window(P, Nb, Nb, cfg.Lbox, R, 8, 0.5 * a, 1)
    exp = w.expected([0])
    S = np.stack([ln.assign(P[0, s], R, cfg.Lbox)[0] for s in range(5)])
    assert S[:, 5].tolist() == [5, 6, 5, 5, 5] and S[:, 20].tolist() == [20, 20, -1, 21, 21] and S[:, 40].tolist() == [-1, 40, 41, 41, 41]
    assert exp["hop1"].tolist() == [3] and exp["hopw"].tolist() == [1] and exp["nlost"].tolist() == [2]
    got = _run(gpu_lib, cfg, P, R, 8, 0.5 * a, Nb, 1, [None])
    _assert_same(got, exp, f"hops dim {dim}")
    assert got["hop1"].tolist() == [2 + 0 + 1] and got["hopw"].tolist() == [0 + 1 + 0]


# ---- 3. lists, launches, resets, neighbours ------------------------------------------------------------------------------
def _small(dim=3, Np=64, Nb=2, W=3, seed=3):
    cfg = _cfg(dim, Np, Nb)
    R, a = _lattice(cfg, Np)
    return cfg, R, a, ln.jittered(R, W, 2 * Nb + 1, Np, cfg.Lbox, np.random.default_rng(seed), 0.2 * a)


def test_walker_listed_twice(gpu_lib):
    cfg, R, a, P = _small()
    once = _run(gpu_lib, cfg, P, R, 10, 0.4 * a, 2, 1, [[0, 1, 2]])
    twice = _run(gpu_lib, cfg, P, R, 10, 0.4 * a, 2, 1, [[0, 0, 1, 2, 2]])
    for k in ln.INT_KEYS + ("mom",):
        for w, f in ((0, 2), (1, 1), (2, 2)):
            assert same_bits(twice[k][w], f * once[k][w]) if k == "mom" else np.array_equal(twice[k][w], f * once[k][w]), (k, w)


def test_launch_split_at_256_walkers(gpu_lib):
    """300 walkers of an Np = 3, Nb = 1 system: two launches; every walker has what a call with it alone gives."""
    W, Nb = 300, 1
    cfg = _cfg(3, 3, Nb)
    R, a = _lattice(cfg, 3)
    P = ln.jittered(R, W, 3, 3, cfg.Lbox, np.random.default_rng(300), 0.2 * a)
    VT, WF = gpu_lib.build_tables(cfg)
    with gpu_lib.PigsContext(cfg, VT, WF, n_walkers=W) as ctx:
        ctx.upload_all(P)
        ctx.lat_init(R, 6, 0.4 * a, Nb, 1)
        ctx.lat_accumulate()
        allw = ctx.lat_read(reset=True)
        for w in range(W):
            ctx.lat_accumulate([w])
        each = ctx.lat_read()
    exp = ln.Window(P, Nb, Nb, cfg.Lbox, R, 6, 0.4 * a, 1).expected(range(W))
    _assert_same(allw, exp, "300 walkers")
    for k in ln.INT_KEYS:
        assert np.array_equal(allw[k], each[k]), k
    assert same_bits(allw["mom"], each["mom"]) and allw["samples"].tolist() == [1] * W


def test_reset_mask(gpu_lib):
    cfg, R, a, P = _small()
    VT, WF = gpu_lib.build_tables(cfg)
    with gpu_lib.PigsContext(cfg, VT, WF, n_walkers=3) as ctx:
        ctx.upload_all(P)
        ctx.lat_init(R, 10, 0.4 * a, 1, 1)
        ctx.lat_accumulate()
        first = ctx.lat_read(reset=[0, 1, 0])
        again = ctx.lat_read()
        ctx.lat_accumulate()
        last = ctx.lat_read(reset=True)
        zero = ctx.lat_read()
    for k in ln.INT_KEYS + ("mom",):
        assert np.array_equal(again[k][[0, 2]], first[k][[0, 2]]) and not np.any(again[k][1]), k
        assert np.array_equal(last[k][[0, 2]], 2 * first[k][[0, 2]]) and np.array_equal(last[k][1], first[k][1]), k
        assert not np.any(zero[k]), k


def test_interleaved_with_grv(gpu_lib):
    """pigs_grv_accumulate between two pigs_lat_accumulate on one context: each family keeps the bits it has alone."""
    cfg, R, a, P = _small()
    VT, WF = gpu_lib.build_tables(cfg)

    def run(lat, grv):
        with gpu_lib.PigsContext(cfg, VT, WF, n_walkers=3) as ctx:
            ctx.upload_all(P)
            if lat:
                ctx.lat_init(R, 10, 0.4 * a, 2, 1)
            if grv:
                ctx.grv_init(8, 2)
            for _ in range(2):
                if lat:
                    ctx.lat_accumulate()
                if grv:
                    ctx.grv_accumulate([2, 0])
            return (ctx.lat_read() if lat else None), (ctx.grv_read() if grv else None)

    lat_alone, _ = run(True, False)
    _, grv_alone = run(False, True)
    lat_both, grv_both = run(True, True)
    for k in ln.INT_KEYS:
        assert np.array_equal(lat_both[k], lat_alone[k]), k
    assert same_bits(lat_both["mom"], lat_alone["mom"]) and lat_both["samples"].tolist() == [2, 2, 2]
    for k in grv_alone:
        assert np.array_equal(grv_both[k], grv_alone[k]), k


# ---- 4. refusals ------------------------------------------------------------------------------------------------------
def test_status_codes(gpu_lib):
    Nb = 3
    ARG, OK, UNS = ST["PIGS_ERR_ARG"], ST["PIGS_OK"], ST["PIGS_ERR_UNSUPPORTED"]
    cfg = _cfg(2, 30, Nb)
    R, a = _lattice(cfg, 30)
    bad = R.copy()
    bad[4, 1] = np.inf
    nan = R.copy()
    nan[0, 0] = np.nan
    VT, WF = gpu_lib.build_tables(cfg)
    with gpu_lib.PigsContext(cfg, VT, WF, n_walkers=2) as ctx:
        init = lambda n, S, nbin, rmax, win, cm: ctx.L.pigs_lat_init(ctx.h, n, S.ctypes.data_as(_dp), nbin, rmax, win, cm)
        assert ctx.L.pigs_lat_accumulate(ctx.h, 1, None) == ARG           # before init
        with pytest.raises(gpu_lib.PigsError):
            ctx.lat_read()
        for args in ((0, R, 8, a, 0, 1), (-1, R, 8, a, 0, 1), (30, bad, 8, a, 0, 1), (30, nan, 8, a, 0, 1), (30, R, 0, a, 0, 1),
                     (30, R, 8, 0.0, 0, 1), (30, R, 8, -a, 0, 1), (30, R, 8, np.inf, 0, 1), (30, R, 8, np.nan, 0, 1),
                     (30, R, 8, a, -1, 1), (30, R, 8, a, Nb + 1, 1), (30, R, 8, a, 0, 2), (30, R, 8, a, 0, -1)):
            assert init(*args) == ARG, args[0:1] + args[2:]
            assert ctx.L.pigs_lat_accumulate(ctx.h, 1, None) == ARG
        assert init(30, R, 8, a, Nb, 0) == OK and init(31, R[:1].repeat(31, 0).copy(), 8, a, 0, 1) == OK
        assert ctx.L.pigs_lat_accumulate(ctx.h, -1, None) == ARG
        assert ctx.L.pigs_lat_accumulate(ctx.h, 1, np.array([2], np.int32).ctypes.data_as(C.POINTER(C.c_int32))) == ARG
        assert init(30, R, 4000, a, 0, 1) == ARG                          # the histograms pass the LDS limit
        ctx.sync()
    # Np and nsite of 1077 are each served in 3D
    for Np, nsite in ((1077, 5), (5, 1077)):
        big = _cfg(3, Np, 1)
        S = ln.grid_sites(3, 11, big.Lbox, nsite)
        VT, WF = gpu_lib.build_tables(big)
        with gpu_lib.PigsContext(big, VT, WF, n_walkers=1) as ctx:
            assert ctx.L.pigs_lat_init(ctx.h, nsite, S.ctypes.data_as(_dp), 100, 1.0, 0, 1) == OK
            ctx.sync()
    # dim = 1 and trapped contexts: unsupported, a status of its own
    one = SystemConfig(dim=1, Np=6, Nb=2, density=0.2)
    tcfg = SystemConfig(dim=2, Np=6, Nb=2, trap=True, a_ho=[1.0, 1.3], Nmax=2000, Rm=1.2, dt=0.01)
    for c in (one, tcfg):
        VT, WF = gpu_lib.build_tables(c)
        with gpu_lib.PigsContext(c, VT, WF, n_walkers=1) as ctx:
            S = np.zeros((6, c.dim))
            assert ctx.L.pigs_lat_init(ctx.h, 6, S.ctypes.data_as(_dp), 8, 1.0, 0, 1) == UNS
            ctx.sync()


def test_nearest_neighbour_distance_of_the_test_lattice():
    cfg = _cfg(3, 64, 1)
    R, a = _lattice(cfg, 64)
    assert abs(nearest_neighbour_distance(R, cfg.Lbox) - a) < 1e-12 * a


# ---- 5. the front end ---------------------------------------------------------------------------------------------------
PRINT = 1.0000001e-9            # the files carry 10 significant digits
LIND = ("u2_mean", "gamma", "alpha2", "vacant", "multiple", "hops_link", "hops_window")


@pytest.fixture(scope="module")
def exe(gpu_lib):
    import subprocess
    host = os.path.join(ROOT, "pathintegralgroundstate_amd", "host")
    subprocess.check_call(["make", "-s", "-C", host])
    return os.path.join(host, "pigs_vpi")


def _crystal(tmp_path, name):
    import shutil
    from test_gpu_front_end_blocks import RUNS
    d = str(tmp_path / name)
    os.makedirs(d)
    shutil.copy(os.path.join(RUNS, "he4_crystal", "config_ini.in"), d)
    return d


def test_front_end_two_blocks_three_steps(gpu_lib, oracle, exe, tmp_path):
    """he4_crystal (27 particles started on the sites of config_ini.in, worm sector on), 2 blocks x 3 steps, two walkers,
    lattice = T with a window of 2: every file of the run without the key byte for byte, with either sampler; the three
    new files of every walker against a replay of the run's chains through PigsContext.lat_* and normalize_lat; two shards
    on one GPU give one shard's per-walker files byte for byte."""
    from test_gpu_front_end_blocks import RUNS, _input, _run as run_vpi, replay
    W, Nblock, Nstep, window, nbin = 2, 2, 3, 2, 16
    txt, _ = _input("he4_crystal", Nblock, Nstep)
    ini = open(os.path.join(RUNS, "he4_crystal", "config_ini.in")).read().split("\n")
    cfg = SystemConfig.from_namelists(txt, Np=int(ini[0]), density=float(ini[2]), Lbox=[float(x) for x in ini[1].split()])
    R = np.array([[float(x) for x in l.split()] for l in ini[3:3 + int(ini[0])]])
    assert R.shape == (cfg.Np, cfg.dim)
    ann = nearest_neighbour_distance(R, cfg.Lbox)
    rmax, ns = 0.5 * ann, 2 * window + 1
    key = f", lattice = T, lat_window = {window}, lat_nbin = {nbin}"
    rep = replay(gpu_lib, oracle, cfg, W, Nblock, Nstep, start=R)
    VT, WF = gpu_lib.build_tables(cfg)
    blocks = []
    with gpu_lib.PigsContext(cfg, VT, WF, n_walkers=W) as ctx:
        ctx.lat_init(R, nbin, rmax, window, 1)
        for b in range(Nblock):
            for t in range(b * Nstep, (b + 1) * Nstep):
                ctx.upload_all(rep["snaps"][t])
                wl = np.nonzero(rep["diag"][t])[0]
                if len(wl):
                    ctx.lat_accumulate(wl)
            blocks.append(ctx.lat_read(reset=True))
    counted = np.stack([b["samples"] > 0 for b in blocks], axis=1)           # [W, Nblock]
    assert counted.any()
    with np.errstate(all="ignore"):
        norm = [normalize_lat_(b, cfg.Np, len(R), ann, rmax) for b in blocks]
    first = None
    for ds in ("T", "F"):
        plain, on = _crystal(tmp_path, "plain" + ds), _crystal(tmp_path, "on" + ds)
        run_vpi(exe, txt + f"&gpu\n n_walkers = {W}, device_sampler = {ds}\n/\n", plain)
        out = run_vpi(exe, txt + f"&gpu\n n_walkers = {W}, device_sampler = {ds}{key}\n/\n", on)
        assert "Lattice sites" in out
        old = sorted(os.listdir(plain))
        new = sorted(set(os.listdir(on)) - set(old))
        assert sorted(f for f in new if ".w" not in f) == ["lind_vpi.out", "lindtau_vpi.out", "usite_vpi.out"], new
        assert len(new) == 3 + 3 * W, new
        for f in old:
            if f not in ("stdout.txt", "vpi.in"):
                assert open(os.path.join(plain, f), "rb").read() == open(os.path.join(on, f), "rb").read(), f
        final = np.fromfile(os.path.join(on, "worldlines_final.bin")).reshape(rep["final"].shape)
        assert np.array_equal(final, rep["final"])
        names = sorted(f for f in new if re.fullmatch(r"lind_vpi\.w\d+\.out", f))
        assert len(names) == W
        for w, fl in enumerate(names):
            bs = [b for b in range(Nblock) if counted[w, b]]
            blk = np.loadtxt(os.path.join(on, fl), ndmin=2)
            assert blk.shape == (len(bs), 8) and blk[:, 0].tolist() == [b + 1.0 for b in bs], (fl, blk.shape)
            if not bs:
                continue
            want = np.array([[norm[b][k][w] for k in LIND] for b in bs])
            scale = np.abs(want)
            scale[:, 2] += 1.0
            assert np.all(np.abs(blk[:, 1:] - want) <= PRINT * scale + 1e-12), (fl, blk[:, 1:] - want)
            assert np.all(want[:, 0] > 0) and np.all(want[:, 1] < 0.5)
            tau = np.loadtxt(os.path.join(on, fl.replace("lind_", "lindtau_")), ndmin=2)
            assert tau.shape == (ns, 3 + cfg.dim)
            assert np.allclose(tau[:, 0], (np.arange(ns) - window) * cfg.dt, rtol=PRINT, atol=1e-300)
            assert np.allclose(tau[:, 1], np.mean([norm[b]["u2"][w] for b in bs], axis=0), rtol=10 * PRINT, atol=0)
            assert np.allclose(tau[:, 2:2 + cfg.dim], np.mean([norm[b]["uk2"][w] for b in bs], axis=0), rtol=10 * PRINT, atol=0)
            assert np.allclose(tau[:, 2 + cfg.dim], np.mean([norm[b]["gamma_tau"][w] for b in bs], axis=0), rtol=10 * PRINT, atol=0)
            us = np.loadtxt(os.path.join(on, fl.replace("lind_", "usite_")), ndmin=2)
            assert us.shape == (nbin, 2 + 2 * cfg.dim)
            assert np.allclose(us[:, 1], np.mean([norm[b]["rho_site"][w] for b in bs], axis=0), rtol=10 * PRINT, atol=1e-300)
            pu = np.mean([norm[b]["pu"][w] for b in bs], axis=0)
            for k in range(cfg.dim):
                assert np.allclose(us[:, 2 + 2 * k], pu[k, nbin - 1::-1], rtol=10 * PRINT, atol=1e-300)
                assert np.allclose(us[:, 3 + 2 * k], pu[k, nbin:], rtol=10 * PRINT, atol=1e-300)
        if first is None:
            first = on
        else:                                                           # the two samplers give the same files
            for f in new:
                assert open(os.path.join(first, f), "rb").read() == open(os.path.join(on, f), "rb").read(), f
    two = _crystal(tmp_path, "two")
    run_vpi(exe, txt + f"&gpu\n n_walkers = {W}, device_sampler = T, device = 0, n_gpus = 2, same_device = T{key}\n/\n", two)
    for f in sorted(os.listdir(first)):
        if ".w" in f and f.endswith(".out"):
            assert open(os.path.join(first, f), "rb").read() == open(os.path.join(two, f), "rb").read(), f


def normalize_lat_(raw, Np, nsite, ann, rmax):
    from pathintegralgroundstate_amd.profiles import normalize_lat
    return normalize_lat(raw, Np, nsite, ann, rmax)


def test_front_end_refuses_a_bad_window_before_any_gpu_work(gpu_lib, exe, tmp_path):
    import subprocess
    from test_gpu_front_end_blocks import _input
    txt, _ = _input("he4_crystal", 1, 1)
    wd = _crystal(tmp_path, "bad")
    with open(os.path.join(wd, "vpi.in"), "w") as f:
        f.write(txt + "&gpu\n lattice = T, lat_window = 1000\n/\n")
    with open(os.path.join(wd, "vpi.in")) as fin:
        r = subprocess.run([exe], stdin=fin, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, cwd=wd, timeout=120)
    out = r.stdout.decode(errors="replace")
    assert r.returncode == 2 and "lattice" in out and "lat_window" in out, out[-2000:]
