"""The self part of F(q,tau) and the imaginary-time displacement on the MI355X (pigs_fqs_*, pigs_fqs.hip), through the C
ABI.

The expected sums come from the numpy restatement in tests/fqs_numpy.py: the full phase per (vector, particle, slice),
nothing factorised, fqv_numpy's loop over (lag, pair), the two-compare fold.  Bounds per element and call:
F 1e-12 * n_pairs(l) * Np, D 1e-12 * the sum of the terms (every shape here keeps Np * (2 W + 1) <= 4000).  No comparison
masks or skips elements.  Every case prints its worst error/bound ratio."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, ROOT
from helpers import same_bits
from pathintegralgroundstate_amd import SystemConfig
from pathintegralgroundstate_amd.profiles import normalize_fqs, normalize_msd, shell_average
from fqs_numpy import expected, n_pairs, n_vectors, vectors

pytestmark = pytest.mark.gpu
RUNS = os.path.join(GOLDEN, "vpi_runs")
HOST = os.path.join(ROOT, "pathintegralgroundstate_amd", "host")
DENSITY = {1: 0.2, 2: 0.25, 3: 0.365}


def _status_codes():
    txt = open(os.path.join(ROOT, "include", "pigs_hip.h")).read()
    return {k: int(v) for k, v in re.findall(r"^\s*(PIGS_\w+)\s*=\s*(-?\d+)", txt, flags=re.M)}


ST = _status_codes()
assert ST["PIGS_OK"] == 0 and len({ST["PIGS_ERR_ARG"], ST["PIGS_ERR_HIP"], ST["PIGS_ERR_UNSUPPORTED"]}) == 3


def _cfg(dim, Np, Nb, **kw):
    return SystemConfig(dim=dim, Np=Np, Nb=Nb, density=DENSITY[dim], **kw)


def _random_paths(cfg, W, rng):
    L = np.asarray(cfg.Lbox[:cfg.dim])
    return rng.uniform(-0.5, 0.5, (W,) + tuple(cfg.path_shape)) * L


def _assert_close(got, want, bound, what=""):
    assert got.shape == want.shape, (got.shape, want.shape)
    err = np.abs(got - want)
    # (an element with want = bound = 0 must be exactly 0: its ratio counts as 0, or inf if not)
    ratio = np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0))
    worst = float(np.max(ratio))
    print(f"{what}: max |got-want|/bound = {worst:.3e} over {got.size} elements")
    assert np.all(np.isfinite(got)) and np.all(err <= bound), (what, worst)
    return worst


def _assert_matches(got, e, what):
    assert got["F"].dtype == np.float64 and got["D"].dtype == np.float64 and got["samples"].dtype == np.int64
    assert np.array_equal(got["samples"], e["samples"])
    _assert_close(got["F"], e["F"], e["Fb"], what + " F")
    _assert_close(got["D"], e["D"], e["Db"], what + " D")


# ---- 1. against the numpy restatement ---------------------------------------------------------------------------------
# (nmax, window, Ntau): one slice; window = Nb with every lag; 0 < Ntau < 2 window.  In 3D nmax 1, 2, 3 give 13, 62 and
# 171 vectors, none a multiple of a tile width; Np 5 is a partial wave, 67 more than one 64-lane pass, 257 beyond 256.
# (Np = 1 is not a case: pigs_ctx_create refuses Np < 2.)
GRIDS = [(1, 0, 0), (2, 4, 8), (3, 3, 2)]


@pytest.mark.parametrize("Np", [5, 67, 257])
@pytest.mark.parametrize("dim", [1, 2, 3])
def test_matches_numpy_on_uploaded_worldlines(gpu_lib, dim, Np):
    W, Nb = 2, 4
    cfg = _cfg(dim, Np, Nb)
    VT, WF = gpu_lib.build_tables(cfg)
    rng = np.random.default_rng(100000 * dim + 100 * Np + 11)
    P = _random_paths(cfg, W, rng)
    with gpu_lib.PigsContext(cfg, VT, WF, n_walkers=W) as ctx:
        ctx.upload_all(P)
        for nmax, window, Ntau in GRIDS:
            ctx.fqs_init(nmax, Ntau, window)
            n = ctx.fqs_vectors()
            assert n.shape == (n_vectors(dim, nmax), dim) and n.dtype == np.int32
            assert np.array_equal(n, vectors(dim, nmax))              # the restatement's own enumeration
            ctx.fqs_accumulate()
            got = ctx.fqs_read()
            assert got["F"].shape == (W, Ntau + 1, n.shape[0]) and got["D"].shape == (W, Ntau + 1, 2)
            e = expected(P, range(W), Nb, window, Ntau, n, cfg.Lbox)
            _assert_matches(got, e, f"dim {dim} Np {Np} nmax {nmax} W {window} Ntau {Ntau}")
            # sum rule: F_s(q, 0) = 1 and <dr^2>(0) = 0 (exactly: lag 0 adds 0.0)
            Fs = normalize_fqs(got["F"], got["samples"], Np, window)
            assert np.all(np.abs(Fs[:, 0] - 1.0) <= 1e-12)
            assert not got["D"][:, 0].any()
            msd, _ = normalize_msd(got["D"], got["samples"], Np, window, dim)
            assert not msd[:, 0].any() and np.all(msd[:, 1:] > 0)


@pytest.mark.parametrize("dim,Np,Nb,nmax,window,Ntau", [
    (2, 5, 24, 4, 24, 48),        # 49 lags: more than 4 lag groups x 12 registers, so tiles of 32 vectors and 8 lag groups
                                  # (40 vectors: the second tile is partial); with 3 lags the same shape runs in tiles of 64
    (2, 5, 10, 64, 10, 3),        # the phasor table of 21 slices at nmax 64 leaves room for 32 vectors: 54.4 KiB of LDS
    (3, 6, 40, 2, 40, 80)])       # 81 lags: tiles of 32; 62 vectors, so the second tile is partial
def test_narrow_tiles_match_numpy(gpu_lib, dim, Np, Nb, nmax, window, Ntau):
    """Shapes at which the kernel takes tiles narrower than 64 vectors (more lags than 48, or a large phasor table)."""
    W = 2
    assert Np * (2 * window + 1) <= 4000
    cfg = _cfg(dim, Np, Nb)
    VT, WF = gpu_lib.build_tables(cfg)
    P = _random_paths(cfg, W, np.random.default_rng(1000 * dim + Ntau))
    with gpu_lib.PigsContext(cfg, VT, WF, n_walkers=W) as ctx:
        ctx.upload_all(P)
        ctx.fqs_init(nmax, Ntau, window)
        n = ctx.fqs_vectors()
        ctx.fqs_accumulate()
        got = ctx.fqs_read()
        # the same sums with fewer lags run in tiles of 64: an element's bits do not involve the tile width
        ctx.fqs_init(nmax, min(Ntau, 2), window)
        ctx.fqs_accumulate()
        few = ctx.fqs_read()
    _assert_matches(got, expected(P, range(W), Nb, window, Ntau, n, cfg.Lbox), f"narrow dim {dim} nmax {nmax} Ntau {Ntau}")
    nl = few["F"].shape[1]
    assert same_bits(few["F"], got["F"][:, :nl]) and same_bits(few["D"], got["D"][:, :nl])


def _k6_context(gpu_lib, oracle, cfg, W):
    from oracle.pyoracle import System
    S = System(dim=cfg.dim, Np=cfg.Np, Nb=cfg.Nb, density=cfg.density, dt=cfg.dt, trap=cfg.trap,
               a_ho=cfg.a_ho, Lbox=cfg.Lbox, rcut=cfg.rcut)
    VT, WF = gpu_lib.build_tables(cfg)
    ctx = gpu_lib.PigsContext(cfg, VT, WF, n_walkers=W)
    ctx.sampler_init()
    Paths = []
    for w in range(W):
        P, g = oracle.init_path(S, cfg.seed + w)
        Paths.append(P)
        ctx.sampler_set_rng(w, g.mti, np.array(g.mt[:], np.uint32))
    ctx.upload_all(np.stack(Paths))
    return ctx


def _he4_cfg():
    return SystemConfig.from_namelists(open(os.path.join(RUNS, "he4_bis_cworm0_s1982", "vpi.in")).read())


# ---- 2. a sampled state ---------------------------------------------------------------------------------------------------
def test_matches_numpy_on_a_sampled_state(gpu_lib, oracle):
    """A state evolved by three K6 steps, accumulated every step."""
    cfg = _he4_cfg()
    W, Nb = 4, cfg.Nb
    assert cfg.Np * (2 * Nb + 1) <= 4000
    ctx = _k6_context(gpu_lib, oracle, cfg, W)
    try:
        nmax, window, Ntau = 3, Nb, Nb
        ctx.fqs_init(nmax, Ntau, window)
        n = ctx.fqs_vectors()
        tot = None
        for istep in range(1, 4):
            ctx.sampler_step(istep)
            ctx.fqs_accumulate()
            e = expected(ctx.download_all(), range(W), Nb, window, Ntau, n, cfg.Lbox)
            tot = e if tot is None else {k: tot[k] + e[k] for k in e}
        got = ctx.fqs_read()
        assert got["samples"].tolist() == [3] * W
        _assert_matches(got, tot, f"sampled nmax {nmax} W {window} Ntau {Ntau}")
    finally:
        ctx.close()


# ---- 3. closed forms ----------------------------------------------------------------------------------------------------
def _lattice(cfg, m):
    dim = cfg.dim
    L = np.asarray(cfg.Lbox[:dim])
    g = np.stack(np.meshgrid(*([np.arange(m)] * dim), indexing="ij"), axis=-1).reshape(-1, dim)
    return -0.5 * L + (g + 0.25) * (L / m), L


@pytest.mark.parametrize("dim,m,nmax", [(3, 4, 3), (2, 9, 5), (1, 7, 9)])
def test_identical_slices(gpu_lib, dim, m, nmax):
    """Every slice the same lattice: F = n_pairs * Np within the bound and D is exactly 0.0."""
    Np, Nb, window = m ** dim, 3, 2
    Ntau = 2 * window
    cfg = _cfg(dim, Np, Nb)
    base, L = _lattice(cfg, m)
    P = np.broadcast_to(base, (1,) + tuple(cfg.path_shape)).copy()
    VT, WF = gpu_lib.build_tables(cfg)
    with gpu_lib.PigsContext(cfg, VT, WF, n_walkers=1) as ctx:
        ctx.upload_all(P)
        ctx.fqs_init(nmax, Ntau, window)
        ctx.fqs_accumulate()
        got = ctx.fqs_read()
    pairs = n_pairs(window, Ntau).astype(np.float64)[:, None]
    want = np.broadcast_to(pairs * Np, got["F"][0].shape)
    _assert_close(got["F"][0], want, 1e-12 * want, f"identical slices dim {dim}")
    assert not got["D"].any() and got["samples"].tolist() == [1]


@pytest.mark.parametrize("dim,m,nmax", [(3, 4, 3), (2, 9, 5), (1, 7, 9)])
def test_rigid_shift_with_wrap(gpu_lib, dim, m, nmax):
    """Slice a+1 is slice a shifted rigidly by delta and folded back into the box, and some particles wrap inside the
    window: F_s(q, l) = Np n_pairs cos(l q.delta) within the bound, D[l][0] = n_pairs Np |l delta|^2 within its bound.
    (tests/test_fqs_host.py checks both on the numpy side alone.)"""
    Np, Nb, window = m ** dim, 4, 3
    Ntau = 4
    cfg = _cfg(dim, Np, Nb)
    base, L = _lattice(cfg, m)
    delta = np.array([0.61, -0.43, 0.37])[:dim] * (L / 7.0)
    assert np.all(np.abs(Ntau * delta) < 0.5 * L - 1e-6 * L)             # |l delta_k| < L/2, and not near it
    b = np.arange(2 * Nb + 1, dtype=np.float64)[:, None, None]
    path = np.mod(base[None] + b * delta[None, None, :] + 0.5 * L, L) - 0.5 * L
    assert np.any(np.abs(np.diff(path[Nb - window:Nb + window + 1], axis=0)) > 0.5 * L)      # wraps inside the window
    VT, WF = gpu_lib.build_tables(cfg)
    with gpu_lib.PigsContext(cfg, VT, WF, n_walkers=1) as ctx:
        ctx.upload_all(path[None])
        ctx.fqs_init(nmax, Ntau, window)
        n = ctx.fqs_vectors()
        ctx.fqs_accumulate()
        got = ctx.fqs_read()
    pairs = n_pairs(window, Ntau).astype(np.float64)
    l = np.arange(Ntau + 1, dtype=np.float64)
    qd = (n * (2.0 * np.pi / L)) @ delta
    want = Np * pairs[:, None] * np.cos(l[:, None] * qd[None, :])
    _assert_close(got["F"][0], want, 1e-12 * pairs[:, None] * Np * np.ones_like(want), f"rigid shift dim {dim} F")
    r2 = pairs * Np * l * l * (delta @ delta)
    _assert_close(got["D"][0, :, 0], r2, 1e-12 * r2, f"rigid shift dim {dim} D")
    msd, a2 = normalize_msd(got["D"][0], 1, Np, window, dim)
    assert np.allclose(msd, l * l * (delta @ delta), rtol=1e-12, atol=0)


# ---- 4. determinism and independence of the launch --------------------------------------------------------------------
def test_bits_do_not_depend_on_the_launch(gpu_lib):
    W, Nb, nmax, window, Ntau = 6, 5, 3, 3, 4
    cfg = _cfg(3, 257, Nb)
    VT, WF = gpu_lib.build_tables(cfg)
    P = _random_paths(cfg, W, np.random.default_rng(5))

    def run(lists, paths=P, nw=W):
        with gpu_lib.PigsContext(cfg, VT, WF, n_walkers=nw) as ctx:
            ctx.upload_all(paths)
            ctx.fqs_init(nmax, Ntau, window)
            for wl in lists:
                ctx.fqs_accumulate(wl)
            return ctx.fqs_read()

    def same(x, y, ix=slice(None), iy=slice(None)):
        return same_bits(x["F"][ix], y["F"][iy]) and same_bits(x["D"][ix], y["D"][iy])

    a = run([None])
    b = run([None])                                         # a fresh context
    assert same(a, b) and a["samples"].tolist() == [1] * W
    assert np.all(np.isfinite(a["F"])) and np.all(a["F"][:, 0] > 0) and np.all(a["D"][:, 1:] > 0)
    singly = run([[w] for w in range(W)])                   # one walker at a time
    assert same(singly, a) and singly["samples"].tolist() == [1] * W
    perm = run([[4, 1, 5, 0, 3, 2]])                        # a permuted list
    assert same(perm, a)
    sub = run([[4, 1]])                                     # a subset, out of order
    assert same(sub, a, [1, 4], [1, 4]) and not sub["F"][[0, 2, 3, 5]].any() and not sub["D"][[0, 2, 3, 5]].any()
    assert sub["samples"].tolist() == [0, 1, 0, 0, 1, 0]
    dup = run([[2, 0, 2]])                                  # listed twice: counts twice
    assert same_bits(dup["F"][2], 2.0 * a["F"][2]) and same_bits(dup["D"][2], 2.0 * a["D"][2]) and same(dup, a, 0, 0)
    assert dup["samples"].tolist() == [1, 0, 2, 0, 0, 0]
    one = run([None], paths=P[2:3], nw=1)                   # the same worldline alone in a second, smaller context
    assert same(one, a, 0, 2)


def test_more_than_256_walkers_in_one_list(gpu_lib):
    """A 600-walker context (three launches behind one call) against the same worldlines six at a time."""
    W, Nb, nmax, window, Ntau = 600, 3, 2, 2, 3
    cfg = _cfg(2, 4, Nb)
    VT, WF = gpu_lib.build_tables(cfg)
    P6 = _random_paths(cfg, 6, np.random.default_rng(11))
    P = P6[np.arange(W) % 6]
    with gpu_lib.PigsContext(cfg, VT, WF, n_walkers=6) as ctx:
        ctx.upload_all(P6)
        ctx.fqs_init(nmax, Ntau, window)
        n = ctx.fqs_vectors()
        ctx.fqs_accumulate()
        small = ctx.fqs_read()
    with gpu_lib.PigsContext(cfg, VT, WF, n_walkers=W) as ctx:
        ctx.upload_all(P)
        ctx.fqs_init(nmax, Ntau, window)
        ctx.fqs_accumulate()
        big = ctx.fqs_read()
        assert big["samples"].tolist() == [1] * W
        assert same_bits(big["F"], small["F"][np.arange(W) % 6]) and same_bits(big["D"], small["D"][np.arange(W) % 6])
        ctx.fqs_accumulate(list(range(W - 1, -1, -1)) + [7, 7, 500])      # 603 entries, with repeats
        big2 = ctx.fqs_read()
        cnt = np.ones(W)
        cnt[7] += 2
        cnt[500] += 1
        assert big2["samples"].tolist() == (cnt + 1).astype(int).tolist()
        for key in ("F", "D"):
            want = np.stack([sum([small[key][w % 6]] * int(cnt[w]), big[key][w]) for w in range(W)])
            assert same_bits(big2[key], want), key
    _assert_matches(small, expected(P6, range(6), Nb, window, Ntau, n, cfg.Lbox), "600-walker shapes")


# ---- 5. stream order ----------------------------------------------------------------------------------------------------
def test_accumulate_sees_the_worldline_queued_before_it(gpu_lib, oracle):
    cfg = _he4_cfg()
    W, Nb, nmax, window = 4, cfg.Nb, 2, min(3, cfg.Nb)
    Ntau = 2 * window
    A = _k6_context(gpu_lib, oracle, cfg, W)
    B = _k6_context(gpu_lib, oracle, cfg, W)
    try:
        A.fqs_init(nmax, Ntau, window)
        n = A.fqs_vectors()
        A.sampler_step(1)
        A.fqs_accumulate()
        A.sampler_step(2)
        got = A.fqs_read()
        B.sampler_step(1)
        P1 = B.download_all()
        B.fqs_init(nmax, Ntau, window)
        B.fqs_accumulate()
        twin = B.fqs_read()
        assert same_bits(got["F"], twin["F"]) and same_bits(got["D"], twin["D"])      # the twin that stopped after step 1
        e1 = expected(P1, range(W), Nb, window, Ntau, n, cfg.Lbox)
        _assert_matches(got, e1, "step 1's worldline")
        B.sampler_step(2)
        e2 = expected(B.download_all(), range(W), Nb, window, Ntau, n, cfg.Lbox)
        assert np.any(np.abs(e2["F"] - e1["F"]) > 10 * e1["Fb"])          # the second step moved the sums: the check has teeth
        assert np.any(np.abs(e2["D"] - e1["D"]) > 10 * e1["Db"])
    finally:
        A.close()
        B.close()


# ---- 6. reset mask, re-init, refusals -------------------------------------------------------------------------------------
def test_reset_mask_reinit_and_status_codes(gpu_lib):
    W, Nb = 3, 4
    cfg = _cfg(2, 40, Nb)
    VT, WF = gpu_lib.build_tables(cfg)
    P = _random_paths(cfg, W, np.random.default_rng(3))
    dp, lp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int64), C.POINTER(C.c_int32)
    with gpu_lib.PigsContext(cfg, VT, WF, n_walkers=W) as ctx:
        ctx.upload_all(P)
        ARG = ST["PIGS_ERR_ARG"]
        # before init
        for call in (ctx.fqs_accumulate, ctx.fqs_read, ctx.fqs_vectors):
            with pytest.raises(gpu_lib.PigsError):
                call()
        assert ctx.L.pigs_fqs_accumulate(ctx.h, 1, None) == ARG
        F1, D1 = np.zeros(1), np.zeros(2)
        cnt = np.zeros(W, np.int64)
        nq = C.c_int64(0)
        nbuf = np.zeros(8, np.int32)
        assert ctx.L.pigs_fqs_read(ctx.h, F1.ctypes.data_as(dp), D1.ctypes.data_as(dp), cnt.ctypes.data_as(lp), None) == ARG
        assert ctx.L.pigs_fqs_count(ctx.h, C.byref(nq)) == ARG
        assert ctx.L.pigs_fqs_vectors(ctx.h, nbuf.ctypes.data_as(ip)) == ARG
        # bad arguments (2D: nmax 1..64): those of pigs_fqv_init; and init stays undone
        for nmax, Ntau, window in ((0, 0, 0), (-2, 0, 0), (65, 0, 0), (5, 0, -1), (5, 0, Nb + 1), (5, -1, 2), (5, 5, 2),
                                   (5, 1, 0)):
            assert ctx.L.pigs_fqs_init(ctx.h, nmax, Ntau, window) == ARG, (nmax, Ntau, window)
            assert ctx.L.pigs_fqv_init(ctx.h, nmax, Ntau, window) == ARG, (nmax, Ntau, window)
            with pytest.raises(gpu_lib.PigsError):
                ctx.fqs_init(nmax, Ntau, window)
        assert ctx.L.pigs_fqs_accumulate(ctx.h, 1, None) == ARG
        # the limits themselves are accepted
        ctx.fqs_init(64, 0, 0)
        ctx.fqs_init(1, 2 * Nb, Nb)
        ctx.fqs_init(3, 4, 2)
        n = ctx.fqs_vectors()
        assert ctx.L.pigs_fqs_count(ctx.h, C.byref(nq)) == ST["PIGS_OK"] and nq.value == n_vectors(2, 3)
        assert ctx.L.pigs_fqs_count(ctx.h, None) == ARG and ctx.L.pigs_fqs_vectors(ctx.h, None) == ARG
        for bad in ([3], [-1], [0, 5], list(range(W)) + [W]):
            with pytest.raises(gpu_lib.PigsError):
                ctx.fqs_accumulate(bad)
        assert ctx.L.pigs_fqs_accumulate(ctx.h, -1, None) == ARG
        wl = np.array([0, W], np.int32)
        assert ctx.L.pigs_fqs_accumulate(ctx.h, 2, wl.ctypes.data_as(ip)) == ARG
        big, bigd = np.zeros(W * 5 * n.shape[0]), np.zeros(W * 5 * 2)
        assert ctx.L.pigs_fqs_read(ctx.h, None, bigd.ctypes.data_as(dp), cnt.ctypes.data_as(lp), None) == ARG
        assert ctx.L.pigs_fqs_read(ctx.h, big.ctypes.data_as(dp), None, cnt.ctypes.data_as(lp), None) == ARG
        assert ctx.L.pigs_fqs_read(ctx.h, big.ctypes.data_as(dp), bigd.ctypes.data_as(dp), None, None) == ARG
        assert ctx.L.pigs_fqs_accumulate(ctx.h, W, None) == ST["PIGS_OK"]       # the context still works
        ctx.fqs_read(reset=True)
        z = ctx.fqs_read()
        assert not z["F"].any() and not z["D"].any() and not z["samples"].any()  # a refused list adds nothing
        # reset mask
        ctx.fqs_accumulate()
        ctx.fqs_accumulate([1])
        e = expected(P, [0, 1, 2, 1], Nb, 2, 4, n, cfg.Lbox)
        got = ctx.fqs_read(reset=[1, 0, 1])
        assert got["samples"].tolist() == [1, 2, 1]
        _assert_matches(got, e, "before reset")
        after = ctx.fqs_read()
        assert after["samples"].tolist() == [0, 2, 0]
        assert same_bits(after["F"][1], got["F"][1]) and same_bits(after["D"][1], got["D"][1])
        assert not after["F"][[0, 2]].any() and not after["D"][[0, 2]].any()
        ctx.fqs_accumulate([0])
        again = ctx.fqs_read(reset=True)
        assert same_bits(again["F"][0], got["F"][0]) and same_bits(again["D"][0], got["D"][0])
        assert again["samples"].tolist() == [1, 2, 0]
        z = ctx.fqs_read()
        assert not z["F"].any() and not z["D"].any() and not z["samples"].any()
        # a second init resizes and zeroes
        ctx.fqs_accumulate()
        ctx.fqs_init(2, 1, 1)
        z = ctx.fqs_read()
        assert z["F"].shape == (W, 2, 12) and z["D"].shape == (W, 2, 2)
        assert not z["F"].any() and not z["D"].any() and not z["samples"].any()
        ctx.fqs_accumulate([2])
        _assert_matches(ctx.fqs_read(), expected(P, [2], Nb, 1, 1, ctx.fqs_vectors(), cfg.Lbox), "after re-init")
    # 3D: nmax stops at 16
    cfg3 = _cfg(3, 8, 2)
    VT, WF = gpu_lib.build_tables(cfg3)
    with gpu_lib.PigsContext(cfg3, VT, WF, n_walkers=1) as ctx:
        assert ctx.L.pigs_fqs_init(ctx.h, 17, 0, 0) == ST["PIGS_ERR_ARG"]
        ctx.fqs_init(16, 4, 2)
        assert ctx.fqs_vectors().shape == (n_vectors(3, 16), 3)
    # accumulators beyond 2 GiB: 3 000 walkers x 5 lags x 17 968 vectors x 8 bytes; the context then still works
    with gpu_lib.PigsContext(cfg3, VT, WF, n_walkers=3000) as ctx:
        assert ctx.L.pigs_fqs_init(ctx.h, 16, 4, 2) == ST["PIGS_ERR_ARG"]
        assert ctx.L.pigs_fqs_accumulate(ctx.h, 1, None) == ST["PIGS_ERR_ARG"]
        ctx.fqs_init(2, 4, 2)
        ctx.fqs_accumulate([2999])
        assert ctx.fqs_read()["samples"][2999] == 1
    # a trapped context: unsupported, a status of its own
    tcfg = SystemConfig(dim=2, Np=6, Nb=2, trap=True, a_ho=[1.0, 1.3], Nmax=2000, Rm=1.2, dt=0.01)
    VT, WF = gpu_lib.build_tables(tcfg)
    with gpu_lib.PigsContext(tcfg, VT, WF, n_walkers=1) as ctx:
        assert ctx.L.pigs_fqs_init(ctx.h, 5, 0, 0) == ST["PIGS_ERR_UNSUPPORTED"]
        assert ctx.L.pigs_fqs_accumulate(ctx.h, 1, None) == ST["PIGS_ERR_ARG"]          # still before init
        with pytest.raises(gpu_lib.PigsError, match="periodic"):
            ctx.fqs_init(5, 0, 0)
        ctx.sync()                                                                      # the context still works


# ---- 7. the front end -------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def exe(gpu_lib):
    subprocess.check_call(["make", "-s", "-C", HOST])
    return os.path.join(HOST, "pigs_vpi")


def _run(exe, txt, wd, expect_rc=0):
    os.makedirs(wd, exist_ok=True)
    with open(os.path.join(wd, "vpi.in"), "w") as f:
        f.write(txt)
    with open(os.path.join(wd, "vpi.in")) as fin, open(os.path.join(wd, "stdout.txt"), "w") as fo:
        r = subprocess.run([exe], stdin=fin, stdout=fo, stderr=subprocess.STDOUT, cwd=wd, timeout=900)
    out = open(os.path.join(wd, "stdout.txt")).read()
    assert r.returncode == expect_rc, out[-3000:]
    return out


def _files(d):
    return sorted(f for f in os.listdir(d) if f not in ("stdout.txt", "vpi.in"))


def _same(a, b, f):
    return open(os.path.join(a, f), "rb").read() == open(os.path.join(b, f), "rb").read()


PRINT = 1.0000001e-9            # the files carry 10 significant digits
NEW = ["fqself_vpi.out", "fqssh_vpi.out", "msd_vpi.out"]


@pytest.mark.parametrize("ds", ["T", "F"])
def test_front_end_one_sample_equals_numpy(exe, tmp_path, ds):
    """One block of one step: the single sample is taken on the worldline that the run then dumps, so numpy on
    worldlines_final.bin is the whole expectation.  Bound: the kernel's, normalised, plus one unit of the last printed
    digit.  fqs_window is left out: ceiling(fqs_ntau/2)."""
    txt = open(os.path.join(RUNS, "he4_bis_cworm0_s1982", "vpi.in")).read()
    cfg = SystemConfig.from_namelists(txt)
    txt = re.sub(r"Nstep\s*=\s*\d+", "Nstep = 1", re.sub(r"Nblock\s*=\s*\d+", "Nblock = 1", txt))
    nmax, Ntau, window = 3, 3, 2
    d = str(tmp_path)
    out = _run(exe, txt + f"&gpu\n device_sampler = {ds}, fq_self = T, fqs_nmax = {nmax}, fqs_ntau = {Ntau}\n/\n", d)
    banner = [ln for ln in out.splitlines() if ln.startswith("  > Self F_s(q,tau)     : on (")]
    assert len(banner) == 1 and f"Nb-{window}..Nb+{window}" in banner[0] and f"lags 0..{Ntau}" in banner[0]
    P = np.fromfile(os.path.join(d, "worldlines_final.bin")).reshape((1,) + tuple(cfg.path_shape))
    n = vectors(cfg.dim, nmax)
    Nq, dim = n.shape[0], cfg.dim
    e = expected(P, [0], cfg.Nb, window, Ntau, n, cfg.Lbox)
    norm = n_pairs(window, Ntau).astype(np.float64) * float(cfg.Np)
    tab = np.loadtxt(os.path.join(d, "fqself_vpi.out"))
    assert tab.shape == ((Ntau + 1) * Nq, dim + 5)
    assert np.array_equal(tab[:, 0], np.repeat(np.arange(Ntau + 1), Nq))                  # lags slowest
    assert np.allclose(tab[:, 1], tab[:, 0] * cfg.dt, rtol=PRINT, atol=0)
    assert np.array_equal(tab[:, 2:2 + dim], np.tile(n, (Ntau + 1, 1)))
    want = e["F"][0] / norm[:, None]
    got = tab[:, 3 + dim].reshape(Ntau + 1, Nq)
    _assert_close(got, want, e["Fb"][0] / norm[:, None] + PRINT * np.abs(want), f"front end F_s, one sample, ds {ds}")
    assert np.all(np.abs(got[0] - 1.0) <= 1e-12 + PRINT)                                  # F_s(q, 0) = 1
    sh = np.loadtxt(os.path.join(d, "fqssh_vpi.out"))
    q, mean, mult = shell_average(n, cfg.Lbox, got)
    assert sh.shape == ((Ntau + 1) * q.size, 6)
    assert np.allclose(sh[:, 2], np.tile(q, Ntau + 1), rtol=PRINT, atol=0)
    assert np.array_equal(sh[:, 5], np.tile(mult, Ntau + 1)) and int(mult.sum()) == 2 * Nq
    tol = PRINT * (np.abs(mean) + shell_average(n, cfg.Lbox, np.abs(got))[1])
    assert np.all(np.abs(sh[:, 3].reshape(Ntau + 1, q.size) - mean) <= tol)
    # msd_vpi.out: l, tau_l, <dr^2>, error, alpha_2
    msd = np.loadtxt(os.path.join(d, "msd_vpi.out"))
    assert msd.shape == (Ntau + 1, 5) and np.array_equal(msd[:, 0], np.arange(Ntau + 1))
    assert np.allclose(msd[:, 1], msd[:, 0] * cfg.dt, rtol=PRINT, atol=0)
    wm, wa = normalize_msd(e["D"][0], 1, cfg.Np, window, dim)
    _assert_close(msd[:, 2], wm, e["Db"][0, :, 0] / norm + PRINT * np.abs(wm), f"front end msd, ds {ds}")
    assert msd[0, 2] == 0.0 and msd[0, 4] == 0.0 and np.all(msd[1:, 2] > 0)
    # alpha_2 + 1 is a quotient of sums each within 1e-12 relative, printed with 10 digits
    assert np.all(np.abs(msd[1:, 4] - wa[1:]) <= (4e-12 + PRINT) * (np.abs(wa[1:]) + 1.0))


@pytest.mark.parametrize("ds", ["T", "F"])
def test_front_end_writes_the_files_and_changes_nothing_else(exe, tmp_path, ds):
    txt = open(os.path.join(RUNS, "he4_worm_s1982", "vpi.in")).read()
    nmax, Ntau, window = 2, 2, 2
    plain, off, on = (str(tmp_path / x) for x in ("plain", "off", "on"))
    out_plain = _run(exe, txt + f"&gpu\n device_sampler = {ds}\n/\n", plain)
    out_off = _run(exe, txt + f"&gpu\n device_sampler = {ds}, fq_self = F, fqs_nmax = 3, fqs_ntau = 2\n/\n", off)
    out = _run(exe, txt + f"&gpu\n device_sampler = {ds}, fq_self = T, fqs_nmax = {nmax}, fqs_ntau = {Ntau}, "
               f"fqs_window = {window}\n/\n", on)
    assert "Self F_s(q,tau)" in out and "Self F_s(q,tau)" not in out_off and "Self F_s(q,tau)" not in out_plain
    old = _files(plain)
    assert _files(off) == old and not set(NEW) & set(old)
    assert _files(on) == sorted(old + NEW)
    for f in old:
        assert _same(plain, off, f), f                     # key off: byte-identical to a run without it
        assert _same(plain, on, f), f                      # key on: nothing else moves
    strip = lambda s: [ln for ln in s.splitlines() if "Time per block" not in ln and "host threads" not in ln]
    assert strip(out_plain) == strip(out_off)
    assert [ln for ln in strip(out) if "Self F_s(q,tau)" not in ln] == strip(out_plain)
    Nq = n_vectors(3, nmax)
    tab = np.loadtxt(os.path.join(on, "fqself_vpi.out"))
    assert tab.shape[0] == (Ntau + 1) * Nq and np.all(np.isfinite(tab)) and np.all(tab[:, -1] >= 0)
    assert np.all(np.abs(tab[:Nq, -2] - 1.0) <= 1e-9)      # F_s(q, 0) = 1 in every block
    msd = np.loadtxt(os.path.join(on, "msd_vpi.out"))
    assert msd.shape == (Ntau + 1, 5) and msd[0, 2] == 0.0 and np.all(np.diff(msd[:, 2]) > 0) and np.all(np.isfinite(msd))


def test_front_end_sharded_contexts_one_gpu(exe, tmp_path):
    """n_walkers = 4 on two contexts of this GPU against one context: per-walker files byte-identical, the
    walker-averaged files equal up to summation order (the block values meet in the all-reduced block vector, behind
    the imaginary-time-profile entries when both keys are on)."""
    txt = open(os.path.join(RUNS, "he4_worm_s1982", "vpi.in")).read()
    key = "tau_profile = T, fq_vector = T, fqv_nmax = 2, fqv_ntau = 2, fqv_window = 1, fq_self = T, fqs_nmax = 2, fqs_ntau = 2, fqs_window = 1"
    a, b = str(tmp_path / "one"), str(tmp_path / "sharded")
    _run(exe, txt + f"&gpu\n n_walkers = 4, device = 0, n_gpus = 1, {key}\n/\n", a)
    _run(exe, txt + f"&gpu\n n_walkers = 4, device = 0, n_gpus = 2, same_device = T, {key}\n/\n", b)
    for w in range(4):
        for f in ("fqself_vpi", "fqssh_vpi", "msd_vpi", "fqvec_vpi", "tau_vpi", "e_vpi"):
            assert _same(a, b, f"{f}.w{w:04d}.out"), (f, w)
    Nq = n_vectors(3, 2)
    # (file, rows, column of the means, column of the errors, derived columns)
    for f, nrow, mean, err, derived in (("fqself_vpi.out", 3 * Nq, [6], [7], []), ("fqssh_vpi.out", None, [3], [4], []),
                                        ("msd_vpi.out", 3, [2], [3], [4]), ("fqvec_vpi.out", 3 * Nq, [6], [7], [])):
        x, y = np.loadtxt(os.path.join(a, f)), np.loadtxt(os.path.join(b, f))
        assert x.shape == y.shape and (nrow is None or x.shape[0] == nrow)
        assert np.all(np.isfinite(x)) and np.all(np.isfinite(y))
        d = np.abs(x - y)
        other = [c for c in range(x.shape[1]) if c not in mean + err + derived]
        assert np.all(d[:, other] == 0), f                 # lags, tau, vectors, |q|, multiplicities
        # means: sums of four walkers' block values in another order, printed with 10 digits; errors: the root of a
        # difference of two moments (test_gpu_fqt.py has the reasoning)
        mtol = PRINT * np.abs(x[:, mean])
        assert np.all(d[:, mean] <= mtol), f
        assert np.all(d[:, err] <= np.sqrt(4.0 * np.abs(x[:, mean]) * mtol) + PRINT * np.abs(x[:, err])), f
        for c in derived:                                  # alpha_2 + 1: a quotient of two such means and a square
            assert np.all(d[:, c] <= 4.0 * PRINT * (np.abs(x[:, c]) + 1.0)), f


def test_front_end_refuses_the_key_for_a_trapped_system(exe, tmp_path):
    txt = open(os.path.join(RUNS, "trap2d_bis_cworm0", "vpi.in")).read()
    out = _run(exe, txt + "&gpu\n fq_self = T\n/\n", str(tmp_path), expect_rc=2)
    assert "fq_self" in out and "periodic" in out
    assert _files(str(tmp_path)) == []


def test_front_end_refuses_out_of_range_keys(exe, tmp_path):
    txt = open(os.path.join(RUNS, "he4_worm_s1982", "vpi.in")).read()                      # 3D, Nb = 8
    for i, (extra, word) in enumerate(((", fqs_nmax = 17", "fqs_nmax"), (", fqs_nmax = 0", "fqs_nmax"),
                                       (", fqs_ntau = -1", "fqs_ntau"), (", fqs_ntau = 5, fqs_window = 2", "fqs_ntau"),
                                       (", fqs_window = 9", "fqs_window"), (", fqs_ntau = 17", "fqs_window"))):
        out = _run(exe, txt + f"&gpu\n fq_self = T{extra}\n/\n", str(tmp_path / str(i)), expect_rc=2)
        assert "fq_self" in out and word in out
        assert _files(str(tmp_path / str(i))) == []
