"""F(q,tau) on the full reciprocal grid on the MI355X (pigs_fqv_*, pigs_fqv.hip), through the C ABI.

The expected sums come from the numpy restatement in tests/fqv_numpy.py: sqv_numpy's full phase per (vector, particle),
nothing factorised, and fqt_numpy's loop over (lag, pair).  The bound per (walker, lag, vector) is
1e-12 * sum over the pairs of (|rho(a)| |rho(a+l)| + Np) with rho from the numpy side: the project's S(k) bound as
fqt_numpy applies it.  No comparison masks or skips elements.  Every case prints its worst error/bound ratio."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, ROOT
from helpers import same_bits
from pathintegralgroundstate_amd import SystemConfig
from pathintegralgroundstate_amd.profiles import normalize_fqv, normalize_sqv, shell_average
from fqv_numpy import expected, n_vectors, vectors
import fqt_numpy

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
    # (a walker that was not listed has want = bound = 0 and must be exactly 0: its ratio counts as 0, or inf if not)
    ratio = np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0))
    worst = float(np.max(ratio))
    print(f"{what}: max |got-want|/bound = {worst:.3e} over {got.size} elements")
    assert np.all(np.isfinite(got)) and np.all(err <= bound), (what, worst)
    return worst


def _grids(dim, Nb):
    """(nmax, window, Ntau): one slice; a last lag of one pair; Ntau < 2 window on 665 vectors in 3D (no multiple of a
    tile); the widest window (ns = 161 at Nb = 80: the narrow LDS tile); the largest grid."""
    big = 16 if dim == 3 else 64
    return [(1, 0, 0), (4, 3, 6), (5, 3, 2), (3, Nb, 2 * Nb), (big, 1, 2)]


# ---- 1. against the numpy restatement ---------------------------------------------------------------------------------
@pytest.mark.parametrize("Nb", [4, 80])
@pytest.mark.parametrize("Np", [2, 64, 257, 520])
@pytest.mark.parametrize("dim", [1, 2, 3])
def test_matches_numpy_on_uploaded_worldlines(gpu_lib, dim, Np, Nb):
    W = 2
    cfg = _cfg(dim, Np, Nb)
    VT, WF = gpu_lib.build_tables(cfg)
    rng = np.random.default_rng(100000 * dim + 100 * Np + Nb + 7)
    P = _random_paths(cfg, W, rng)
    with gpu_lib.PigsContext(cfg, VT, WF, n_walkers=W) as ctx:
        ctx.upload_all(P)
        for nmax, window, Ntau in _grids(dim, Nb):
            ctx.fqv_init(nmax, Ntau, window)
            n = ctx.fqv_vectors()
            assert n.shape == (((2 * nmax + 1) ** dim - 1) // 2, dim) and n.dtype == np.int32
            assert np.array_equal(n, vectors(dim, nmax))              # the restatement's own enumeration
            ctx.fqv_accumulate()
            got = ctx.fqv_read()
            F, B, cnt = expected(P, range(W), Nb, window, Ntau, n, cfg.Lbox)
            assert got["F"].shape == (W, Ntau + 1, n.shape[0]) and got["F"].dtype == np.float64
            assert got["samples"].dtype == np.int64 and np.array_equal(got["samples"], cnt)
            _assert_close(got["F"], F, B, f"dim {dim} Np {Np} Nb {Nb} nmax {nmax} W {window} Ntau {Ntau}")


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
    ctx = _k6_context(gpu_lib, oracle, cfg, W)
    try:
        for nmax, window, Ntau in ((4, 3, 6), (8, Nb, Nb)):
            ctx.fqv_init(nmax, Ntau, window)
            n = ctx.fqv_vectors()
            F = np.zeros((W, Ntau + 1, n.shape[0]))
            B = np.zeros_like(F)
            for istep in range(1, 4):
                ctx.sampler_step(istep)
                ctx.fqv_accumulate()
                e = expected(ctx.download_all(), range(W), Nb, window, Ntau, n, cfg.Lbox)
                F, B = F + e[0], B + e[1]
            got = ctx.fqv_read()
            assert got["samples"].tolist() == [3] * W
            _assert_close(got["F"], F, B, f"sampled nmax {nmax} W {window} Ntau {Ntau}")
    finally:
        ctx.close()


# ---- 3. ties to the pinned estimators ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim,Np,nmax", [(3, 257, 5), (2, 300, 20), (1, 5, 64)])
def test_lag_zero_is_sqv_bit_for_bit(gpu_lib, dim, Np, nmax):
    """Lag 0 against sqv_read()["S"] for the same nmax and window; and the sqv bits of a context that never called fqv
    equal those of one that did."""
    W, Nb, window = 3, 6, 3
    cfg = _cfg(dim, Np, Nb)
    VT, WF = gpu_lib.build_tables(cfg)
    P = _random_paths(cfg, W, np.random.default_rng(dim * 1000 + Np + 1))
    with gpu_lib.PigsContext(cfg, VT, WF, n_walkers=W) as ctx:       # never calls fqv
        ctx.upload_all(P)
        ctx.sqv_init(nmax, window)
        ctx.sqv_accumulate()
        alone = ctx.sqv_read()["S"]
    with gpu_lib.PigsContext(cfg, VT, WF, n_walkers=W) as ctx:
        ctx.upload_all(P)
        ctx.fqv_init(nmax, 2 * window, window)
        ctx.sqv_init(nmax, window)
        ctx.fqv_accumulate()
        ctx.sqv_accumulate()
        ctx.fqv_accumulate()
        S = ctx.sqv_read()["S"]
        F = ctx.fqv_read()["F"]
        assert np.array_equal(ctx.fqv_vectors(), ctx.sqv_vectors())
    assert np.all(np.isfinite(S)) and np.all(S > 0)
    assert same_bits(S, alone)
    assert same_bits(F[:, 0], S + S)                                  # two fqv accumulates: exactly 2x
    assert np.allclose(normalize_fqv(F, 2, Np, window)[:, 0], normalize_sqv(S, 1, Np, window), rtol=1e-15, atol=0)


@pytest.mark.parametrize("dim,Np", [(3, 64), (2, 300), (1, 5)])
def test_axis_vectors_are_the_pinned_fqt(gpu_lib, dim, Np):
    """The vectors (n,0,..), (0,n,..), .. at all lags against pigs_fqt_* of the same window, within the bound."""
    W, Nb, window = 3, 6, 3
    Ntau = 2 * window
    nmax = 8 if dim == 3 else 20
    cfg = _cfg(dim, Np, Nb)
    VT, WF = gpu_lib.build_tables(cfg)
    P = _random_paths(cfg, W, np.random.default_rng(dim * 1000 + Np + 2))
    with gpu_lib.PigsContext(cfg, VT, WF, n_walkers=W) as ctx:
        ctx.upload_all(P)
        ctx.fqv_init(nmax, Ntau, window)
        n = ctx.fqv_vectors()
        ctx.fqv_accumulate()
        got = ctx.fqv_read()["F"]                                      # [W, Ntau+1, Nq]
        ctx.fqt_init(nmax, Ntau, window)
        ctx.fqt_accumulate()
        axis_dev = ctx.fqt_read()["F"]                                 # [W, Ntau+1, nmax, dim]
    _, bound, _ = fqt_numpy.expected(P, range(W), Nb, window, Ntau, nmax, cfg.Lbox)
    axis = np.zeros_like(axis_dev)
    for k in range(dim):
        for iq in range(1, nmax + 1):
            v = np.zeros(dim, np.int32)
            v[k] = iq
            hit = np.flatnonzero((n == v).all(axis=1))
            assert hit.size == 1
            axis[:, :, iq - 1, k] = got[:, :, hit[0]]
    _assert_close(axis, axis_dev, bound, f"pigs_fqt, all lags, dim {dim}")


# ---- 4. analytic: a perfect simple-cubic lattice --------------------------------------------------------------------------
@pytest.mark.parametrize("dim,m,nmax", [(3, 4, 8), (2, 16, 32)])
@pytest.mark.parametrize("shift", [0.0, 1.0 / np.sqrt(7.0)])
def test_simple_cubic_lattice(gpu_lib, dim, m, nmax, shift):
    """m^dim particles on a simple-cubic lattice, every slice identical: rho_q = Np e^(i phi) at the stored vectors whose
    components are all multiples of m and 0 elsewhere, so lag l adds Np^2 (ns - l) resp. 0; a rigid shift of the lattice
    by an irrational fraction of the spacing moves nothing."""
    Np, Nb, window = m ** dim, 3, 2
    ns = 2 * window + 1
    Ntau = ns - 1
    cfg = _cfg(dim, Np, Nb)
    L = np.asarray(cfg.Lbox[:dim])
    assert np.all(L == L[0])
    a = L / m
    g = np.stack(np.meshgrid(*([np.arange(m)] * dim), indexing="ij"), axis=-1).reshape(-1, dim)
    base = -0.5 * L + (g + 0.25 + shift) * a
    base = np.where(base >= 0.5 * L, base - L, base)
    P = np.broadcast_to(base, (1,) + tuple(cfg.path_shape)).copy()
    VT, WF = gpu_lib.build_tables(cfg)
    with gpu_lib.PigsContext(cfg, VT, WF, n_walkers=1) as ctx:
        ctx.upload_all(P)
        ctx.fqv_init(nmax, Ntau, window)
        n = ctx.fqv_vectors()
        ctx.fqv_accumulate()
        got = ctx.fqv_read()["F"][0]                                   # [Ntau+1, Nq]
    bragg = (n % m == 0).all(axis=1)
    assert bragg.sum() > 0 and (~bragg).sum() > 0
    pairs = (ns - np.arange(Ntau + 1, dtype=np.float64))[:, None]
    want = pairs * np.where(bragg, float(Np) * Np, 0.0)[None, :]
    bound = 1e-12 * pairs * (np.where(bragg, float(Np) * Np, 0.0) + Np)[None, :]
    _assert_close(got, want, bound, f"lattice dim {dim} shift {shift:.3f}")
    assert np.allclose(normalize_fqv(got, 1, Np, window)[:, bragg], Np, rtol=1e-11)


# ---- 5. determinism and independence of the launch --------------------------------------------------------------------
def test_bits_do_not_depend_on_the_launch(gpu_lib):
    W, Nb, nmax, window, Ntau = 6, 5, 5, 3, 4
    cfg = _cfg(3, 257, Nb)
    VT, WF = gpu_lib.build_tables(cfg)
    P = _random_paths(cfg, W, np.random.default_rng(5))

    def run(lists, paths=P, nw=W):
        with gpu_lib.PigsContext(cfg, VT, WF, n_walkers=nw) as ctx:
            ctx.upload_all(paths)
            ctx.fqv_init(nmax, Ntau, window)
            for wl in lists:
                ctx.fqv_accumulate(wl)
            return ctx.fqv_read()

    a = run([None])
    b = run([None])                                         # a fresh context
    assert same_bits(a["F"], b["F"]) and a["samples"].tolist() == [1] * W
    assert np.all(np.isfinite(a["F"])) and np.all(a["F"][:, 0] > 0) and a["F"][:, 1:].any()
    sub = run([[4, 1]])                                     # a subset, out of order
    assert same_bits(sub["F"][[1, 4]], a["F"][[1, 4]]) and not sub["F"][[0, 2, 3, 5]].any()
    assert sub["samples"].tolist() == [0, 1, 0, 0, 1, 0]
    twice = run([None, None])                               # two accumulates: exactly 2x
    assert same_bits(twice["F"], 2.0 * a["F"]) and twice["samples"].tolist() == [2] * W
    dup = run([[2, 0, 2, 2]])                               # listed three times: counts three times
    assert same_bits(dup["F"][2], a["F"][2] + a["F"][2] + a["F"][2]) and same_bits(dup["F"][0], a["F"][0])
    assert dup["samples"].tolist() == [1, 0, 3, 0, 0, 0]
    one = run([None], paths=P[2:3], nw=1)                   # the same worldline alone in a context of one walker
    assert same_bits(one["F"][0], a["F"][2])


def test_more_than_256_walkers_in_one_list(gpu_lib):
    """A 1 024-walker context (four launches of 256 behind one call) against the same worldlines six at a time."""
    W, Nb, nmax, window, Ntau = 1024, 3, 3, 2, 3
    cfg = _cfg(2, 64, Nb)
    VT, WF = gpu_lib.build_tables(cfg)
    rng = np.random.default_rng(11)
    P6 = _random_paths(cfg, 6, rng)
    P = P6[np.arange(W) % 6]
    with gpu_lib.PigsContext(cfg, VT, WF, n_walkers=6) as ctx:
        ctx.upload_all(P6)
        ctx.fqv_init(nmax, Ntau, window)
        n = ctx.fqv_vectors()
        ctx.fqv_accumulate()
        small = ctx.fqv_read()["F"]
    with gpu_lib.PigsContext(cfg, VT, WF, n_walkers=W) as ctx:
        ctx.upload_all(P)
        ctx.fqv_init(nmax, Ntau, window)
        ctx.fqv_accumulate()
        big = ctx.fqv_read()
        assert big["samples"].tolist() == [1] * W
        assert same_bits(big["F"], small[np.arange(W) % 6])
        ctx.fqv_accumulate(list(range(W - 1, -1, -1)) + [7, 7, 900])      # 1 027 entries, with repeats
        big2 = ctx.fqv_read()
        cnt = np.ones(W)
        cnt[7] += 2
        cnt[900] += 1
        assert big2["samples"].tolist() == (cnt + 1).astype(int).tolist()
        want = np.stack([sum([small[w % 6]] * int(cnt[w]), big["F"][w]) for w in range(W)])
        assert same_bits(big2["F"], want)
    F, B, _ = expected(P6, range(6), Nb, window, Ntau, n, cfg.Lbox)
    _assert_close(small, F, B, "1024-walker shapes")


# ---- 6. stream order ----------------------------------------------------------------------------------------------------
def test_accumulate_sees_the_worldline_queued_before_it(gpu_lib, oracle):
    cfg = _he4_cfg()
    W, Nb, nmax, window = 4, cfg.Nb, 4, min(3, cfg.Nb)
    Ntau = 2 * window
    A = _k6_context(gpu_lib, oracle, cfg, W)
    B = _k6_context(gpu_lib, oracle, cfg, W)
    C_ = _k6_context(gpu_lib, oracle, cfg, W)
    try:
        A.fqv_init(nmax, Ntau, window)
        n = A.fqv_vectors()
        A.sampler_step(1)
        A.fqv_accumulate()
        A.sampler_step(2)
        got = A.fqv_read()
        B.sampler_step(1)
        P1 = B.download_all()
        B.fqv_init(nmax, Ntau, window)
        B.fqv_accumulate()
        twin = B.fqv_read()
        assert same_bits(got["F"], twin["F"])             # the twin that stopped after step 1
        E1, Bd, _ = expected(P1, range(W), Nb, window, Ntau, n, cfg.Lbox)
        _assert_close(got["F"], E1, Bd, "step 1's worldline")
        B.sampler_step(2)
        P2 = B.download_all()
        E2 = expected(P2, range(W), Nb, window, Ntau, n, cfg.Lbox)[0]
        assert np.any(np.abs(E2 - E1) > 10 * Bd)          # the second step moved the sums: the check has teeth
        # beside the asynchronous estimators: their results are the same bits with and without the accumulate
        C_.fqv_init(nmax, Ntau, window)
        C_.sampler_step(1)
        C_.diagonal_estimators_begin(cfg.Nbin, cfg.rbin, cfg.Nk)
        C_.fqv_accumulate()
        C_.sampler_step(2)
        est = C_.diagonal_estimators_end()
        assert same_bits(C_.fqv_read()["F"], got["F"])
        B2 = _k6_context(gpu_lib, oracle, cfg, W)
        try:
            B2.sampler_step(1)
            B2.diagonal_estimators_begin(cfg.Nbin, cfg.rbin, cfg.Nk)
            B2.sampler_step(2)
            ref = B2.diagonal_estimators_end()
        finally:
            B2.close()
        for k in ("E1", "K1", "V1", "E2", "K2", "V2", "Et", "Kt", "Vt", "gr", "Sk"):
            assert same_bits(est[k], ref[k]), k
    finally:
        A.close()
        B.close()
        C_.close()


# ---- 7. reset mask, re-init, refusals -------------------------------------------------------------------------------------
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
        with pytest.raises(gpu_lib.PigsError):
            ctx.fqv_accumulate()
        with pytest.raises(gpu_lib.PigsError):
            ctx.fqv_read()
        with pytest.raises(gpu_lib.PigsError):
            ctx.fqv_vectors()
        assert ctx.L.pigs_fqv_accumulate(ctx.h, 1, None) == ARG
        F1 = np.zeros(1)
        cnt = np.zeros(W, np.int64)
        nq = C.c_int64(0)
        nbuf = np.zeros(8, np.int32)
        assert ctx.L.pigs_fqv_read(ctx.h, F1.ctypes.data_as(dp), cnt.ctypes.data_as(lp), None) == ARG
        assert ctx.L.pigs_fqv_count(ctx.h, C.byref(nq)) == ARG
        assert ctx.L.pigs_fqv_vectors(ctx.h, nbuf.ctypes.data_as(ip)) == ARG
        # bad arguments (2D: nmax 1..64), and init stays undone
        for nmax, Ntau, window in ((0, 0, 0), (-2, 0, 0), (65, 0, 0), (5, 0, -1), (5, 0, Nb + 1), (5, -1, 2), (5, 5, 2),
                                   (5, 1, 0)):
            assert ctx.L.pigs_fqv_init(ctx.h, nmax, Ntau, window) == ARG, (nmax, Ntau, window)
            with pytest.raises(gpu_lib.PigsError):
                ctx.fqv_init(nmax, Ntau, window)
        assert ctx.L.pigs_fqv_accumulate(ctx.h, 1, None) == ARG
        # the limits themselves are accepted
        ctx.fqv_init(64, 0, 0)
        ctx.fqv_init(1, 2 * Nb, Nb)
        ctx.fqv_init(3, 4, 2)
        n = ctx.fqv_vectors()
        assert ctx.L.pigs_fqv_count(ctx.h, C.byref(nq)) == ST["PIGS_OK"] and nq.value == n_vectors(2, 3)
        assert ctx.L.pigs_fqv_count(ctx.h, None) == ARG and ctx.L.pigs_fqv_vectors(ctx.h, None) == ARG
        for bad in ([3], [-1], [0, 5], list(range(W)) + [W]):
            with pytest.raises(gpu_lib.PigsError):
                ctx.fqv_accumulate(bad)
        assert ctx.L.pigs_fqv_accumulate(ctx.h, -1, None) == ARG
        wl = np.array([0, W], np.int32)
        assert ctx.L.pigs_fqv_accumulate(ctx.h, 2, wl.ctypes.data_as(ip)) == ARG
        big = np.zeros(W * 5 * n.shape[0])
        assert ctx.L.pigs_fqv_read(ctx.h, None, cnt.ctypes.data_as(lp), None) == ARG
        assert ctx.L.pigs_fqv_read(ctx.h, big.ctypes.data_as(dp), None, None) == ARG
        assert ctx.L.pigs_fqv_accumulate(ctx.h, W, None) == ST["PIGS_OK"]       # the context still works
        ctx.fqv_read(reset=True)
        assert not ctx.fqv_read()["F"].any()               # a refused list adds nothing
        # reset mask
        ctx.fqv_accumulate()
        ctx.fqv_accumulate([1])
        one = expected(P, [0, 1, 2], Nb, 2, 4, n, cfg.Lbox)
        got = ctx.fqv_read(reset=[1, 0, 1])
        assert got["samples"].tolist() == [1, 2, 1]
        _assert_close(got["F"], one[0] * np.array([1, 2, 1.0])[:, None, None], one[1] * 2, "before reset")
        after = ctx.fqv_read()
        assert after["samples"].tolist() == [0, 2, 0]
        assert same_bits(after["F"][1], got["F"][1]) and not after["F"][[0, 2]].any()
        ctx.fqv_accumulate([0])
        again = ctx.fqv_read(reset=True)
        assert same_bits(again["F"][0], got["F"][0]) and again["samples"].tolist() == [1, 2, 0]
        assert not ctx.fqv_read()["F"].any() and not ctx.fqv_read()["samples"].any()
        # a second init resizes and zeroes
        ctx.fqv_accumulate()
        ctx.fqv_init(2, 1, 1)
        z = ctx.fqv_read()
        assert z["F"].shape == (W, 2, 12) and not z["F"].any() and not z["samples"].any()
        ctx.fqv_accumulate([2])
        e = expected(P, [2], Nb, 1, 1, ctx.fqv_vectors(), cfg.Lbox)
        _assert_close(ctx.fqv_read()["F"], e[0], e[1], "after re-init")
    # 3D: nmax stops at 16
    cfg3 = _cfg(3, 8, 2)
    VT, WF = gpu_lib.build_tables(cfg3)
    with gpu_lib.PigsContext(cfg3, VT, WF, n_walkers=1) as ctx:
        assert ctx.L.pigs_fqv_init(ctx.h, 17, 0, 0) == ST["PIGS_ERR_ARG"]
        ctx.fqv_init(16, 4, 2)
        assert ctx.fqv_vectors().shape == (n_vectors(3, 16), 3)
    # accumulators beyond 2 GiB: 3 000 walkers x 5 lags x 17 968 vectors x 8 bytes; the context then still works
    with gpu_lib.PigsContext(cfg3, VT, WF, n_walkers=3000) as ctx:
        assert ctx.L.pigs_fqv_init(ctx.h, 16, 4, 2) == ST["PIGS_ERR_ARG"]
        assert ctx.L.pigs_fqv_accumulate(ctx.h, 1, None) == ST["PIGS_ERR_ARG"]
        ctx.fqv_init(2, 4, 2)
        ctx.fqv_accumulate([2999])
        assert ctx.fqv_read()["samples"][2999] == 1
    # 1D: nmax up to 64
    cfg1 = _cfg(1, 8, 2)
    VT, WF = gpu_lib.build_tables(cfg1)
    with gpu_lib.PigsContext(cfg1, VT, WF, n_walkers=1) as ctx:
        assert ctx.L.pigs_fqv_init(ctx.h, 65, 0, 0) == ST["PIGS_ERR_ARG"]
        ctx.fqv_init(64, 0, 0)
        assert ctx.fqv_vectors().ravel().tolist() == list(range(1, 65))
    # a trapped context: unsupported, a status of its own
    tcfg = SystemConfig(dim=2, Np=6, Nb=2, trap=True, a_ho=[1.0, 1.3], Nmax=2000, Rm=1.2, dt=0.01)
    VT, WF = gpu_lib.build_tables(tcfg)
    with gpu_lib.PigsContext(tcfg, VT, WF, n_walkers=1) as ctx:
        assert ctx.L.pigs_fqv_init(ctx.h, 5, 0, 0) == ST["PIGS_ERR_UNSUPPORTED"]
        assert ctx.L.pigs_fqv_accumulate(ctx.h, 1, None) == ST["PIGS_ERR_ARG"]          # still before init
        with pytest.raises(gpu_lib.PigsError, match="periodic"):
            ctx.fqv_init(5, 0, 0)
        ctx.sync()                                                                      # the context still works


def test_shell_table_per_lag(gpu_lib):
    """shell_average, unchanged, gives the per-lag, per-shell table: its lag-0 row is sqv's shell table."""
    W, Nb, nmax, window, Ntau = 2, 4, 4, 2, 3
    cfg = _cfg(3, 64, Nb)
    VT, WF = gpu_lib.build_tables(cfg)
    P = _random_paths(cfg, W, np.random.default_rng(17))
    with gpu_lib.PigsContext(cfg, VT, WF, n_walkers=W) as ctx:
        ctx.upload_all(P)
        ctx.fqv_init(nmax, Ntau, window)
        ctx.sqv_init(nmax, window)
        ctx.fqv_accumulate()
        ctx.sqv_accumulate()
        n = ctx.fqv_vectors()
        f = ctx.fqv_read()
        s = ctx.sqv_read()
    q, mean, mult = shell_average(n, cfg.Lbox, normalize_fqv(f["F"], f["samples"], cfg.Np, window))
    q0, mean0, mult0 = shell_average(n, cfg.Lbox, normalize_sqv(s["S"], s["samples"], cfg.Np, window))
    assert mean.shape == (W, Ntau + 1, q.size) and np.array_equal(mult, mult0) and np.array_equal(q, q0)
    assert np.allclose(mean[:, 0], mean0, rtol=1e-15, atol=0)


# ---- 8. the front end -------------------------------------------------------------------------------------------------
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


@pytest.mark.parametrize("ds", ["T", "F"])
def test_front_end_one_sample_equals_numpy(exe, tmp_path, ds):
    """One block of one step: the single sample is taken on the worldline that the run then dumps, so numpy on
    worldlines_final.bin is the whole expectation.  Bound: the kernel's, normalised, plus one unit of the last printed
    digit.  fqv_window is left out: ceiling(fqv_ntau/2)."""
    txt = open(os.path.join(RUNS, "he4_bis_cworm0_s1982", "vpi.in")).read()
    cfg = SystemConfig.from_namelists(txt)
    txt = re.sub(r"Nstep\s*=\s*\d+", "Nstep = 1", re.sub(r"Nblock\s*=\s*\d+", "Nblock = 1", txt))
    nmax, Ntau, window = 4, 3, 2
    d = str(tmp_path)
    out = _run(exe, txt + f"&gpu\n device_sampler = {ds}, fq_vector = T, fqv_nmax = {nmax}, fqv_ntau = {Ntau}\n/\n", d)
    banner = [ln for ln in out.splitlines() if ln.startswith("  > Vector F(q,tau)   : on (")]
    assert len(banner) == 1 and f"Nb-{window}..Nb+{window}" in banner[0] and f"lags 0..{Ntau}" in banner[0]
    P = np.fromfile(os.path.join(d, "worldlines_final.bin")).reshape((1,) + tuple(cfg.path_shape))
    n = vectors(cfg.dim, nmax)
    Nq, dim = n.shape[0], cfg.dim
    A, B, _ = expected(P, [0], cfg.Nb, window, Ntau, n, cfg.Lbox)
    norm = (2 * window + 1 - np.arange(Ntau + 1))[:, None] * float(cfg.Np)
    tab = np.loadtxt(os.path.join(d, "fqvec_vpi.out"))
    assert tab.shape == ((Ntau + 1) * Nq, dim + 5)
    assert np.array_equal(tab[:, 0], np.repeat(np.arange(Ntau + 1), Nq))                  # lags slowest
    assert np.allclose(tab[:, 1], tab[:, 0] * cfg.dt, rtol=PRINT, atol=0)
    assert np.array_equal(tab[:, 2:2 + dim], np.tile(n, (Ntau + 1, 1)))
    qb = 2 * np.pi / np.asarray(cfg.Lbox[:dim])
    assert np.allclose(tab[:, 2 + dim], np.tile(np.sqrt(((n * qb) ** 2).sum(axis=1)), Ntau + 1), rtol=PRINT, atol=0)
    want = A[0] / norm
    got = tab[:, 3 + dim].reshape(Ntau + 1, Nq)
    _assert_close(got, want, B[0] / norm + PRINT * np.abs(want), f"front end, one sample, ds {ds}")
    # the shell file is the shell average of the vector file (means of printed 10-digit values against a printed mean)
    sh = np.loadtxt(os.path.join(d, "fqsh_vpi.out"))
    q, mean, mult = shell_average(n, cfg.Lbox, got)
    assert sh.shape == ((Ntau + 1) * q.size, 6)
    assert np.array_equal(sh[:, 0], np.repeat(np.arange(Ntau + 1), q.size))
    assert np.allclose(sh[:, 1], sh[:, 0] * cfg.dt, rtol=PRINT, atol=0)
    assert np.allclose(sh[:, 2], np.tile(q, Ntau + 1), rtol=PRINT, atol=0)
    assert np.array_equal(sh[:, 5], np.tile(mult, Ntau + 1)) and int(mult.sum()) == 2 * Nq
    # (a mean of values that carry one unit of the tenth digit of the largest of them each)
    tol = PRINT * (np.abs(mean) + shell_average(n, cfg.Lbox, np.abs(got))[1])
    assert np.all(np.abs(sh[:, 3].reshape(Ntau + 1, q.size) - mean) <= tol)


@pytest.mark.parametrize("ds", ["T", "F"])
def test_front_end_writes_the_files_and_changes_nothing_else(exe, tmp_path, ds):
    txt = open(os.path.join(RUNS, "he4_worm_s1982", "vpi.in")).read()
    cfg = SystemConfig.from_namelists(txt)
    nmax, Ntau, window = 3, 2, 2
    plain, off, on, sq = (str(tmp_path / x) for x in ("plain", "off", "on", "sq"))
    out_plain = _run(exe, txt + f"&gpu\n device_sampler = {ds}\n/\n", plain)
    out_off = _run(exe, txt + f"&gpu\n device_sampler = {ds}, fq_vector = F, fqv_nmax = 3, fqv_ntau = 2\n/\n", off)
    out = _run(exe, txt + f"&gpu\n device_sampler = {ds}, fq_vector = T, fqv_nmax = {nmax}, fqv_ntau = {Ntau}, "
               f"fqv_window = {window}\n/\n", on)
    _run(exe, txt + f"&gpu\n device_sampler = {ds}, sq_vector = T, sq_nmax = {nmax}, sq_window = {window}\n/\n", sq)
    assert "Vector F(q,tau)" in out and "Vector F(q,tau)" not in out_off and "Vector F(q,tau)" not in out_plain
    old = _files(plain)
    assert _files(off) == old and "fqvec_vpi.out" not in old and "fqsh_vpi.out" not in old
    assert _files(on) == sorted(old + ["fqsh_vpi.out", "fqvec_vpi.out"])
    for f in old:
        assert _same(plain, off, f), f                     # key off: byte-identical to a run without it
        assert _same(plain, on, f), f                      # key on: nothing else moves
    strip = lambda s: [ln for ln in s.splitlines() if "Time per block" not in ln and "host threads" not in ln]
    assert strip(out_plain) == strip(out_off)
    assert [ln for ln in strip(out) if "Vector F(q,tau)" not in ln] == strip(out_plain)
    # lag 0 is the vector S(q) of the same window: the same bits from the device, the same normalisation, so the
    # printed fields are the same characters
    dim = cfg.dim
    Nq = n_vectors(dim, nmax)
    fv = [ln.split() for ln in open(os.path.join(on, "fqvec_vpi.out"))]
    sv = [ln.split() for ln in open(os.path.join(sq, "sqvec_vpi.out"))]
    assert len(fv) == (Ntau + 1) * Nq and len(sv) == Nq
    assert all(r[0] == "0" and float(r[1]) == 0.0 for r in fv[:Nq])
    assert [r[2:] for r in fv[:Nq]] == sv
    fs = [ln.split() for ln in open(os.path.join(on, "fqsh_vpi.out"))]
    ss = [ln.split() for ln in open(os.path.join(sq, "sq_vpi.out"))]
    assert len(fs) == (Ntau + 1) * len(ss) and [r[2:] for r in fs[:len(ss)]] == ss
    tab = np.loadtxt(os.path.join(on, "fqvec_vpi.out"))
    assert np.all(np.isfinite(tab)) and np.all(tab[:, -1] >= 0) and np.all(tab[:Nq, -2] > 0)


def test_front_end_sharded_contexts_one_gpu(exe, tmp_path):
    """n_walkers = 4 on two contexts of this GPU against one context: per-walker files byte-identical, the
    walker-averaged files equal up to summation order (the block values meet in the all-reduced block vector, behind
    the vector-S(q) entries when both keys are on)."""
    txt = open(os.path.join(RUNS, "he4_worm_s1982", "vpi.in")).read()
    key = "sq_vector = T, sq_nmax = 3, sq_window = 1, fq_vector = T, fqv_nmax = 3, fqv_ntau = 2, fqv_window = 1"
    a, b = str(tmp_path / "one"), str(tmp_path / "sharded")
    _run(exe, txt + f"&gpu\n n_walkers = 4, device = 0, n_gpus = 1, {key}\n/\n", a)
    _run(exe, txt + f"&gpu\n n_walkers = 4, device = 0, n_gpus = 2, same_device = T, {key}\n/\n", b)
    for w in range(4):
        for f in ("fqvec_vpi", "fqsh_vpi", "sqvec_vpi", "sk_vpi", "e_vpi"):
            assert _same(a, b, f"{f}.w{w:04d}.out"), (f, w)
    Nq = n_vectors(3, 3)
    # (file, rows, column of the means, column of the errors)
    for f, nrow, mean, err in (("fqvec_vpi.out", 3 * Nq, [6], [7]), ("fqsh_vpi.out", None, [3], [4]),
                               ("sqvec_vpi.out", Nq, [4], [5])):
        x, y = np.loadtxt(os.path.join(a, f)), np.loadtxt(os.path.join(b, f))
        assert x.shape == y.shape and (nrow is None or x.shape[0] == nrow)
        assert np.all(np.isfinite(x)) and np.all(np.isfinite(y))
        d = np.abs(x - y)
        other = [c for c in range(x.shape[1]) if c not in mean + err]
        assert np.all(d[:, other] == 0), f                 # lags, tau, vectors, |q|, multiplicities
        # means: sums of four walkers' block values in another order, printed with 10 digits; errors: the root of a
        # difference of two moments (test_gpu_fqt.py has the reasoning)
        mtol = PRINT * np.abs(x[:, mean])
        assert np.all(d[:, mean] <= mtol), f
        assert np.all(d[:, err] <= np.sqrt(4.0 * np.abs(x[:, mean]) * mtol) + PRINT * np.abs(x[:, err])), f
    assert np.array_equal(np.loadtxt(os.path.join(b, "fqvec_vpi.out"))[:Nq, 2:5], vectors(3, 3))


def test_front_end_refuses_the_key_for_a_trapped_system(exe, tmp_path):
    txt = open(os.path.join(RUNS, "trap2d_bis_cworm0", "vpi.in")).read()
    out = _run(exe, txt + "&gpu\n fq_vector = T\n/\n", str(tmp_path), expect_rc=2)
    assert "fq_vector" in out and "periodic" in out
    assert _files(str(tmp_path)) == []


def test_front_end_refuses_out_of_range_keys(exe, tmp_path):
    txt = open(os.path.join(RUNS, "he4_worm_s1982", "vpi.in")).read()                      # 3D, Nb = 8
    for i, (extra, word) in enumerate(((", fqv_nmax = 17", "fqv_nmax"), (", fqv_nmax = 0", "fqv_nmax"),
                                       (", fqv_ntau = -1", "fqv_ntau"), (", fqv_ntau = 5, fqv_window = 2", "fqv_ntau"),
                                       (", fqv_window = 9", "fqv_window"), (", fqv_ntau = 17", "fqv_window"))):
        out = _run(exe, txt + f"&gpu\n fq_vector = T{extra}\n/\n", str(tmp_path / str(i)), expect_rc=2)
        assert "fq_vector" in out and word in out
        assert _files(str(tmp_path / str(i))) == []
