"""The per-walker accumulator families on the MI355X where they meet: one context keeps ONE set of launch marks
(csrc/pigs_walker_split.h) for the five families that may not list a walker twice in a launch.  Interleaved calls of
fqt, sqv, tau, fqv and fqs with repeated walkers must leave in every family exactly the bits and sample counts that the
same calls of that family alone leave in a fresh context on the same worldlines.  The same again with bop, atm, nk
(pigs_nk_add), lat and sf, which take launches on the same marks, and grv, vh and g3, which advance the launch counter
without checking it, interleaved between them.  sf is the one family whose kernels also write a scratch of their own
between the launches of a call."""
import numpy as np
import pytest

import lat_numpy
from pathintegralgroundstate_amd import SystemConfig

pytestmark = pytest.mark.gpu

INIT = {"fqt": (3, 2, 1), "tau": (), "sqv": (2, 1), "fqv": (2, 2, 1), "fqs": (2, 2, 1)}     # fqt: Nk, Ntau, window;
CALLS = [("fqt", [2, 0, 2]), ("sqv", [2, 2]), ("tau", [0, 2, 0]), ("fqv", [1, 1, 2]),      # sqv: nmax, window;
         ("fqs", [2, 1, 2]), ("fqt", None)]                                                # fqv, fqs: nmax, Ntau, window


def _run(gpu_lib, cfg, VT, WF, P, families):
    with gpu_lib.PigsContext(cfg, VT, WF, n_walkers=P.shape[0]) as ctx:
        ctx.upload_all(P)
        for f in families:
            getattr(ctx, f + "_init")(*INIT[f])
        for f, walkers in CALLS:
            if f in families:
                getattr(ctx, f + "_accumulate")(walkers)
        return {f: getattr(ctx, f + "_read")() for f in families}


def test_interleaved_families_keep_their_own_bits(gpu_lib):
    W = 3
    cfg = SystemConfig(dim=2, Np=5, Nb=3, density=0.25)
    VT, WF = gpu_lib.build_tables(cfg)
    P = np.random.default_rng(20261019).uniform(-0.5, 0.5, (W,) + tuple(cfg.path_shape)) * np.asarray(cfg.Lbox[:cfg.dim])
    together = _run(gpu_lib, cfg, VT, WF, P, list(INIT))
    listed = {"fqt": [2, 1, 3], "sqv": [0, 0, 2], "tau": [2, 0, 1], "fqv": [0, 2, 1], "fqs": [0, 1, 2]}
    for f in INIT:
        alone = _run(gpu_lib, cfg, VT, WF, P, [f])[f]
        assert sorted(alone) == sorted(together[f])
        assert alone["samples"].tolist() == listed[f]               # a walker listed twice is added twice
        for k, a in alone.items():
            t = together[f][k]
            assert a.shape == t.shape and a.dtype == t.dtype and a.dtype.itemsize == 8, (f, k)
            assert np.any(a != 0), (f, k)
            assert np.array_equal(a.view(np.uint64), t.view(np.uint64)), (f, k)


# bop, atm, nk (through nk_add), lat and sf take launches on the same marks; grv, vh and g3 advance the same launch counter
# and may list a walker twice in a launch.  (walkers, and for nk the samples per listed walker)
MORE = [("bop", [2, 0, 2]), ("grv", [1, 1, 0]), ("lat", [2, 0, 2]), ("fqt", [2, 0, 2]), ("sf", [2, 0, 2]), ("atm", [0, 2, 0]),
        ("vh", [2, 2, 1]), ("nk", [1, 1, 2], [2, 1, 3]), ("sqv", [2, 2]), ("g3", [0, 1, 0, 0]), ("bop", None), ("lat", None),
        ("sf", None), ("tau", [0, 2, 0]), ("atm", [1, 1, 2]), ("nk", [2, 0], [1, 2]), ("fqv", [1, 1, 2]), ("grv", None),
        ("g3", [2, 2]), ("sf", [1, 1, 2]), ("fqs", [2, 1, 2]), ("lat", [2, 2, 1]), ("vh", [0, 0, 0]), ("atm", None),
        ("fqt", None)]
LISTED = {"fqt": [2, 1, 3], "sqv": [0, 0, 2], "tau": [2, 0, 1], "fqv": [0, 2, 1], "fqs": [0, 1, 2], "bop": [2, 1, 3],
          "atm": [3, 3, 3], "grv": [2, 3, 1], "vh": [3, 1, 2], "g3": [3, 1, 2], "nk": [2, 3, 4], "lat": [2, 2, 5],
          "sf": [2, 3, 4]}


def _run_more(gpu_lib, cfg, VT, WF, P, init, pairs, families):
    with gpu_lib.PigsContext(cfg, VT, WF, n_walkers=P.shape[0]) as ctx:
        ctx.upload_all(P)
        for f in families:
            getattr(ctx, f + "_init")(*init[f])
        at = 0
        for f, walkers, *nsamp in MORE:
            if f == "nk":                                           # the same pairs whether nk is alone or not
                n = sum(nsamp[0])
                if f in families:
                    ctx.nk_add(walkers, nsamp[0], pairs[at:at + n])
                at += n
            elif f in families:
                getattr(ctx, f + "_accumulate")(walkers)
        return {f: getattr(ctx, f + "_read")() for f in families}


def test_interleaved_thirteen_families_keep_their_own_bits(gpu_lib):
    """The five families above with bop, atm, nk, lat, sf, grv, vh and g3 between them, walkers repeated within the lists:
    in every family the bits and the sample counts of that family's calls alone in a fresh context.  lat: three calls, one
    of them with every walker, on the first five centres of a 3 x 3 grid, window 2, the centre of mass removed.  sf: three
    calls, one of them with every walker, the lags 0..3 of window 2 (of Nb = 3): fewer lags than the window holds."""
    W = 3
    cfg = SystemConfig(dim=2, Np=5, Nb=3, density=0.25)
    VT, WF = gpu_lib.build_tables(cfg)
    L = np.asarray(cfg.Lbox[:cfg.dim])
    rng = np.random.default_rng(20261020)
    P = rng.uniform(-0.5, 0.5, (W,) + tuple(cfg.path_shape)) * L
    pairs = rng.uniform(-0.5, 0.5, (sum(sum(c[2]) for c in MORE if c[0] == "nk"), 2, cfg.dim)) * L
    init = dict(INIT, bop=(cfg.rcut, 1, 4, 3, cfg.rcut / 3.0), atm=(cfg.rcut, 1), nk=(2, 3), grv=(4, 1, 3, cfg.rcut / 3.0),
                vh=(2, 1, 3, cfg.rcut / 3.0, 4, cfg.rcut / 4.0), g3=(2, cfg.rcut / 2.0, 3, 1),
                lat=(lat_numpy.grid_sites(2, 3, cfg.Lbox, cfg.Np), 4, cfg.rcut, 2, 1), sf=(3, 2))
    assert len(init) == 13 and set(init) == set(LISTED) == {c[0] for c in MORE}
    assert init["lat"][0].shape == (cfg.Np, cfg.dim) and np.all(np.isfinite(init["lat"][0]))
    together = _run_more(gpu_lib, cfg, VT, WF, P, init, pairs, list(init))
    for f in init:
        alone = _run_more(gpu_lib, cfg, VT, WF, P, init, pairs, [f])[f]
        assert sorted(alone) == sorted(together[f])
        assert alone["nopen" if f == "nk" else "samples"].tolist() == LISTED[f], f
        assert any(np.any(a != 0) for k, a in alone.items() if k not in ("samples", "nopen", "window")), f
        for k, a in alone.items():
            t = together[f][k]
            if (f, k) == ("sf", "window"):                          # sf_read's one plain int: the window of sf_init
                assert type(a) is int and type(t) is int and a == t == init["sf"][1]
                continue
            assert a.shape == t.shape and a.dtype == t.dtype and a.dtype.itemsize == 8, (f, k)
            assert np.array_equal(a.view(np.uint64), t.view(np.uint64)), (f, k)
        if f == "sf":
            assert alone["C"].shape == (W, init["sf"][0] + 1, cfg.dim) and np.all(alone["D"][:, 1:] > 0)
