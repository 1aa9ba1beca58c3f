"""The per-walker accumulator families on the MI355X where they meet: one context keeps ONE set of launch marks
(csrc/pigs_walker_split.h) for the five families that may not list a walker twice in a launch.  Interleaved calls of
fqt, sqv, tau, fqv and fqs with repeated walkers must leave in every family exactly the bits and sample counts that the
same calls of that family alone leave in a fresh context on the same worldlines."""
import numpy as np
import pytest

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
