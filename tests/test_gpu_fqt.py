"""Imaginary-time density correlations F(q,tau) of a periodic system on the MI355X (pigs_fqt_*, pigs_fqt.hip), through
the C ABI and the front end.

The expected sums come from the numpy restatement in tests/fqt_numpy.py.  The bound per element is
1e-12 * sum over the pairs of (|rho(a)|*|rho(a+l)| + Np) with |rho| from the numpy side: the project's S(k) bound
1e-12*(|want| + Np) (test_gpu_parity.py::test_structure_estimators_vs_oracle) applied per pair.  No comparison masks or
skips elements: every (walker, l, iq, k) is compared in every case."""
import os
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, ROOT
from fqt_numpy import expected, fqt_sums, n_pairs, rho
from helpers import same_bits, ulp_diff
from pathintegralgroundstate_amd import SystemConfig

pytestmark = pytest.mark.gpu
RUNS = os.path.join(GOLDEN, "vpi_runs")
HOST = os.path.join(ROOT, "pathintegralgroundstate_amd", "host")
DENSITY = {1: 0.2, 2: 0.25, 3: 0.365}


def _status_codes():
    """The pigs_status values as include/pigs_hip.h declares them."""
    import re
    txt = open(os.path.join(ROOT, "include", "pigs_hip.h")).read()
    return {k: int(v) for k, v in re.findall(r"^\s*(PIGS_\w+)\s*=\s*(-?\d+)", txt, flags=re.M)}


ST = _status_codes()
assert ST["PIGS_OK"] == 0 and len({ST["PIGS_ERR_ARG"], ST["PIGS_ERR_HIP"], ST["PIGS_ERR_UNSUPPORTED"]}) == 3


def _cfg(dim, Np, Nb, **kw):
    return SystemConfig(dim=dim, Np=Np, Nb=Nb, density=DENSITY[dim], **kw)


def _random_paths(cfg, W, rng):
    """In-box worldlines: every slice uniform in the box, so |rho_q| ~ sqrt(Np) and the slices are uncorrelated."""
    L = np.asarray(cfg.Lbox[:cfg.dim])
    return rng.uniform(-0.5, 0.5, (W,) + tuple(cfg.path_shape)) * L


def _assert_close(got, want, bound, what=""):
    assert got.shape == want.shape, (got.shape, want.shape)
    err = np.abs(got - want)
    worst = float(np.max(err / bound))
    print(f"{what}: max |got-want|/bound = {worst:.3e} over {got.size} elements")
    assert np.all(np.isfinite(got)) and np.all(err <= bound), (what, worst)


def _windows(Nb):
    return [(0, 0), (3, 6), (3, 2), (Nb, 2 * Nb)]


# ---- 1. against the numpy restatement ---------------------------------------------------------------------------------
@pytest.mark.parametrize("Nb", [4, 80])
@pytest.mark.parametrize("Np", [2, 64, 256, 257, 300])
@pytest.mark.parametrize("dim", [1, 2, 3])
def test_matches_numpy_on_uploaded_worldlines(gpu_lib, dim, Np, Nb):
    W = 3
    cfg = _cfg(dim, Np, Nb)
    VT, WF = gpu_lib.build_tables(cfg)
    rng = np.random.default_rng(100000 * dim + 100 * Np + Nb)
    P = _random_paths(cfg, W, rng)
    with gpu_lib.PigsContext(cfg, VT, WF, n_walkers=W) as ctx:
        ctx.upload_all(P)
        for Nk in (1, 50):
            for window, Ntau in _windows(Nb):
                ctx.fqt_init(Nk, Ntau, window)
                ctx.fqt_accumulate()
                got = ctx.fqt_read()
                F, B, n = expected(P, range(W), Nb, window, Ntau, Nk, cfg.Lbox)
                assert got["F"].shape == (W, Ntau + 1, Nk, dim) and got["samples"].dtype == np.int64
                assert np.array_equal(got["samples"], n)
                _assert_close(got["F"], F, B, f"dim {dim} Np {Np} Nb {Nb} Nk {Nk} W {window} Ntau {Ntau}")


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


def test_matches_numpy_on_a_sampled_state(gpu_lib, oracle):
    """A state evolved by a few sampler steps (correlated slices: the lags carry signal), every step accumulated."""
    cfg = _he4_cfg()
    W, Nb, Nk = 4, cfg.Nb, 50
    ctx = _k6_context(gpu_lib, oracle, cfg, W)
    try:
        for window, Ntau in _windows(Nb):
            window = min(window, Nb)
            Ntau = min(Ntau, 2 * window)
            ctx.fqt_init(Nk, Ntau, window)
            F = np.zeros((W, Ntau + 1, Nk, cfg.dim))
            B = np.zeros_like(F)
            for istep in range(1, 4):
                ctx.sampler_step(istep)
                ctx.fqt_accumulate()
                e = expected(ctx.download_all(), range(W), Nb, window, Ntau, Nk, cfg.Lbox)
                F, B = F + e[0], B + e[1]
            got = ctx.fqt_read()
            assert got["samples"].tolist() == [3] * W
            _assert_close(got["F"], F, B, f"sampled W {window} Ntau {Ntau}")
    finally:
        ctx.close()


# ---- 2. tie to the reference ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim,Np", [(3, 64), (3, 37), (2, 300), (1, 5)])
def test_lag_zero_is_the_structure_factor(gpu_lib, oracle, dim, Np):
    from oracle.pyoracle import System
    W, Nb, Nk = 3, 6, 50
    cfg = _cfg(dim, Np, Nb)
    S = System(dim=dim, Np=Np, Nb=Nb, density=cfg.density)
    assert list(S.Lbox[:dim]) == list(cfg.Lbox[:dim])
    VT, WF = gpu_lib.build_tables(cfg)
    P = _random_paths(cfg, W, np.random.default_rng(dim * 1000 + Np))
    with gpu_lib.PigsContext(cfg, VT, WF, n_walkers=W) as ctx:
        ctx.upload_all(P)
        ctx.fqt_init(Nk, 0, 0)
        ctx.fqt_accumulate()
        got = ctx.fqt_read()["F"]
        _, Sk = ctx.structure_batch(Nb, cfg.Nbin, cfg.rbin, Nk)
        for w in range(W):
            want = np.asarray(oracle.structure_factor(S, Nk, P[w][Nb])).reshape(Nk, dim)
            _assert_close(got[w, 0], want, 1e-12 * (np.abs(want) + Np), "oracle.structure_factor")
            _assert_close(got[w, 0], Sk[w], 1e-12 * (np.abs(want) + Np), "structure_batch")
        # a window: lag 0 is the sum of the window slices' S(k) increments
        window = 3
        ctx.fqt_init(Nk, 2, window)
        ctx.fqt_accumulate()
        got = ctx.fqt_read()["F"]
        tot = np.zeros((W, Nk, dim))
        bound = np.zeros((W, Nk, dim))
        for ib in range(Nb - window, Nb + window + 1):
            Sk = ctx.structure_batch(ib, cfg.Nbin, cfg.rbin, Nk)[1]
            tot += Sk
            C, Sn = rho(P[:, ib], Nk, cfg.Lbox)
            bound += 1e-12 * ((C * C + Sn * Sn) + Np)
        _assert_close(got[:, 0], tot, bound, "window sum of structure_batch")


# ---- 3. analytic case -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim,Np", [(1, 64), (2, 257), (3, 300)])
def test_rigidly_shifted_slices(gpu_lib, dim, Np):
    """Slice s = slice Nb-W shifted by (s-Nb+W)*d: rho_q(s) = rho_q(Nb-W) exp(i q (s-Nb+W) d), so
    acc[l][iq][k] = n_pairs(l) |rho|^2 cos(q l d_k)."""
    Nb, window, Nk = 5, 4, 50
    Ntau = 2 * window
    cfg = _cfg(dim, Np, Nb)
    VT, WF = gpu_lib.build_tables(cfg)
    rng = np.random.default_rng(Np)
    L = np.asarray(cfg.Lbox[:dim])
    base = rng.uniform(-0.5, 0.5, (Np, dim)) * L
    d = np.array([0.013, -0.021, 0.008])[:dim] * L
    P = np.zeros((2,) + tuple(cfg.path_shape))
    for s in range(cfg.path_shape[0]):
        P[0, s] = base + (s - Nb + window) * d
        P[1, s] = base                                     # d = 0
    C, S = rho(base, Nk, cfg.Lbox)
    mod2 = C * C + S * S
    qbin = 2.0 * np.pi / L
    q = np.arange(1, Nk + 1, dtype=np.float64)[:, None] * qbin[None, :]
    npair = n_pairs(window, Ntau).astype(np.float64)
    with gpu_lib.PigsContext(cfg, VT, WF, n_walkers=2) as ctx:
        ctx.upload_all(P)
        ctx.fqt_init(Nk, Ntau, window)
        ctx.fqt_accumulate()
        got = ctx.fqt_read()["F"]
    l = np.arange(Ntau + 1, dtype=np.float64)
    want = npair[:, None, None] * mod2[None] * np.cos(q[None] * l[:, None, None] * d[None, None, :])
    bound = 1e-12 * npair[:, None, None] * (mod2[None] + Np)
    _assert_close(got[0], want, bound, "shifted")
    # d = 0: every pair product is |rho|^2 with the same bits; acc[l]/n_pairs(l) differ by the rounding of the running
    # sum (at most n_pairs - 1 <= 8 additions, each within half an ulp of the running value) and of one division
    per = got[1] / npair[:, None, None]
    u = ulp_diff(per, np.broadcast_to(per[Ntau], per.shape))      # lag 2W has a single pair: the product itself
    print("d = 0: max ulp distance across lags", float(u.max()))
    assert float(u.max()) <= 2 * window + 2
    _assert_close(got[1], npair[:, None, None] * mod2[None], bound, "d = 0")


# ---- 4. determinism and independence of the launch --------------------------------------------------------------------
def test_bits_do_not_depend_on_the_launch(gpu_lib):
    W, Nb, Nk, window, Ntau = 6, 5, 13, 3, 5
    cfg = _cfg(3, 257, Nb)
    VT, WF = gpu_lib.build_tables(cfg)
    P = _random_paths(cfg, W, np.random.default_rng(5))

    def run(lists, paths=P, nw=W):
        with gpu_lib.PigsContext(cfg, VT, WF, n_walkers=nw) as ctx:
            ctx.upload_all(paths)
            ctx.fqt_init(Nk, Ntau, window)
            for wl in lists:
                ctx.fqt_accumulate(wl)
            return ctx.fqt_read()

    a = run([None])
    b = run([None])                                         # a fresh context
    assert same_bits(a["F"], b["F"]) and a["samples"].tolist() == [1] * W
    assert np.all(np.isfinite(a["F"])) and np.all(a["F"][:, 0] > 0)
    sub = run([[4, 1]])                                     # a subset, out of order
    assert same_bits(sub["F"][[1, 4]], a["F"][[1, 4]]) and not sub["F"][[0, 2, 3, 5]].any()
    assert sub["samples"].tolist() == [0, 1, 0, 0, 1, 0]
    twice = run([None, None])                               # two accumulates: exactly 2x
    assert same_bits(twice["F"], 2.0 * a["F"]) and twice["samples"].tolist() == [2] * W
    dup = run([[2, 0, 2, 2]])                               # listed three times: counts three times
    assert same_bits(dup["F"][2], a["F"][2] + a["F"][2] + a["F"][2]) and same_bits(dup["F"][0], a["F"][0])
    assert dup["samples"].tolist() == [1, 0, 3, 0, 0, 0]
    twice_listed = run([[3, 3]])
    assert same_bits(twice_listed["F"][3], 2.0 * a["F"][3]) and twice_listed["samples"][3] == 2


def test_more_than_256_walkers_in_one_list(gpu_lib):
    """A 1 024-walker context (four launches of 256 behind one call) against the same worldlines six at a time."""
    W, Nb, Nk, window, Ntau = 1024, 3, 5, 2, 4
    cfg = _cfg(2, 64, Nb)
    VT, WF = gpu_lib.build_tables(cfg)
    rng = np.random.default_rng(11)
    P6 = _random_paths(cfg, 6, rng)
    P = P6[np.arange(W) % 6]
    with gpu_lib.PigsContext(cfg, VT, WF, n_walkers=6) as ctx:
        ctx.upload_all(P6)
        ctx.fqt_init(Nk, Ntau, window)
        ctx.fqt_accumulate()
        small = ctx.fqt_read()["F"]
    with gpu_lib.PigsContext(cfg, VT, WF, n_walkers=W) as ctx:
        ctx.upload_all(P)
        ctx.fqt_init(Nk, Ntau, window)
        ctx.fqt_accumulate()
        big = ctx.fqt_read()
        assert big["samples"].tolist() == [1] * W
        assert same_bits(big["F"], small[np.arange(W) % 6])
        ctx.fqt_accumulate(list(range(W - 1, -1, -1)) + [7, 7, 900])      # 1 027 entries, with repeats
        big2 = ctx.fqt_read()
        cnt = np.ones(W)
        cnt[7] += 2
        cnt[900] += 1
        assert big2["samples"].tolist() == (cnt + 1).astype(int).tolist()
        want = np.stack([sum([small[w % 6]] * int(cnt[w]), big["F"][w]) for w in range(W)])
        assert same_bits(big2["F"], want)
    F, B, _ = expected(P6, range(6), Nb, window, Ntau, Nk, cfg.Lbox)
    _assert_close(small, F, B, "1024-walker shapes")


# ---- 5. stream order --------------------------------------------------------------------------------------------------
def test_accumulate_sees_the_worldline_queued_before_it(gpu_lib, oracle):
    cfg = _he4_cfg()
    W, Nb, Nk, window, Ntau = 4, cfg.Nb, 50, min(3, cfg.Nb), 4
    A = _k6_context(gpu_lib, oracle, cfg, W)
    B = _k6_context(gpu_lib, oracle, cfg, W)
    C_ = _k6_context(gpu_lib, oracle, cfg, W)
    try:
        A.fqt_init(Nk, Ntau, window)
        A.sampler_step(1)
        A.fqt_accumulate()
        A.sampler_step(2)
        got = A.fqt_read()
        B.sampler_step(1)
        P1 = B.download_all()
        B.fqt_init(Nk, Ntau, window)
        B.fqt_accumulate()
        twin = B.fqt_read()
        assert same_bits(got["F"], twin["F"])             # the twin that stopped after step 1
        F, Bd, _ = expected(P1, range(W), Nb, window, Ntau, Nk, cfg.Lbox)
        _assert_close(got["F"], F, Bd, "step 1's worldline")
        B.sampler_step(2)
        P2 = B.download_all()
        F2 = expected(P2, range(W), Nb, window, Ntau, Nk, cfg.Lbox)[0]
        assert np.any(np.abs(F2 - F) > 10 * Bd)           # the second step moved the sums: the check has teeth
        # beside the asynchronous estimators: their results are the same bits with and without the accumulate
        C_.fqt_init(Nk, Ntau, window)
        C_.sampler_step(1)
        C_.diagonal_estimators_begin(cfg.Nbin, cfg.rbin, cfg.Nk)
        C_.fqt_accumulate()
        C_.sampler_step(2)
        est = C_.diagonal_estimators_end()
        assert same_bits(C_.fqt_read()["F"], got["F"])
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


# ---- 6. reset mask, re-init; 7. status codes ----------------------------------------------------------------------------
def test_reset_mask_reinit_and_status_codes(gpu_lib):
    W, Nb = 3, 4
    cfg = _cfg(2, 40, Nb)
    VT, WF = gpu_lib.build_tables(cfg)
    P = _random_paths(cfg, W, np.random.default_rng(3))
    with gpu_lib.PigsContext(cfg, VT, WF, n_walkers=W) as ctx:
        ctx.upload_all(P)
        # before init
        with pytest.raises(gpu_lib.PigsError):
            ctx.fqt_accumulate()
        rc0 = ctx.L.pigs_fqt_accumulate(ctx.h, 1, None)
        assert rc0 == ST["PIGS_ERR_ARG"]
        F = np.zeros(1)
        n = np.zeros(W, np.int64)
        import ctypes as C
        assert ctx.L.pigs_fqt_read(ctx.h, F.ctypes.data_as(C.POINTER(C.c_double)), n.ctypes.data_as(C.POINTER(C.c_int64)), None) == rc0
        # bad arguments: all the same status (PIGS_ERR_ARG), and init stays undone
        for Nk, Ntau, window in ((0, 0, 0), (-2, 0, 0), (5, 0, -1), (5, 0, Nb + 1), (5, -1, 2), (5, 5, 2), (5, 1, 0)):
            assert ctx.L.pigs_fqt_init(ctx.h, Nk, Ntau, window) == rc0, (Nk, Ntau, window)
            with pytest.raises(gpu_lib.PigsError):
                ctx.fqt_init(Nk, Ntau, window)
        assert ctx.L.pigs_fqt_accumulate(ctx.h, 1, None) == rc0
        # the limits themselves are accepted
        ctx.fqt_init(1, 2 * Nb, Nb)
        ctx.fqt_init(7, 4, 2)
        for bad in ([3], [-1], [0, 5], list(range(W)) + [W]):
            with pytest.raises(gpu_lib.PigsError):
                ctx.fqt_accumulate(bad)
        assert ctx.L.pigs_fqt_accumulate(ctx.h, -1, None) == rc0
        wl = np.array([0, W], np.int32)
        assert ctx.L.pigs_fqt_accumulate(ctx.h, 2, wl.ctypes.data_as(C.POINTER(C.c_int32))) == ST["PIGS_ERR_ARG"]
        assert ctx.L.pigs_fqt_read(ctx.h, None, n.ctypes.data_as(C.POINTER(C.c_int64)), None) == ST["PIGS_ERR_ARG"]
        assert ctx.L.pigs_fqt_accumulate(ctx.h, W, None) == ST["PIGS_OK"]
        ctx.fqt_read(reset=True)
        assert not ctx.fqt_read()["F"].any()               # a refused list adds nothing
        # reset mask
        ctx.fqt_accumulate()
        ctx.fqt_accumulate([1])
        one = expected(P, [0, 1, 2], Nb, 2, 4, 7, cfg.Lbox)
        got = ctx.fqt_read(reset=[1, 0, 1])
        assert got["samples"].tolist() == [1, 2, 1]
        _assert_close(got["F"], one[0] * np.array([1, 2, 1.0])[:, None, None, None], one[1] * 2, "before reset")
        after = ctx.fqt_read()
        assert after["samples"].tolist() == [0, 2, 0]
        assert same_bits(after["F"][1], got["F"][1]) and not after["F"][[0, 2]].any()
        ctx.fqt_accumulate([0])
        again = ctx.fqt_read(reset=True)
        assert same_bits(again["F"][0], got["F"][0]) and again["samples"].tolist() == [1, 2, 0]
        assert not ctx.fqt_read()["F"].any() and not ctx.fqt_read()["samples"].any()
        # a second init resizes and zeroes
        ctx.fqt_accumulate()
        ctx.fqt_init(3, 1, 1)
        z = ctx.fqt_read()
        assert z["F"].shape == (W, 2, 3, 2) and not z["F"].any() and not z["samples"].any()
        ctx.fqt_accumulate([2])
        e = expected(P, [2], Nb, 1, 1, 3, cfg.Lbox)
        _assert_close(ctx.fqt_read()["F"], e[0], e[1], "after re-init")
    # a trapped context: unsupported, a status of its own
    tcfg = SystemConfig(dim=2, Np=6, Nb=2, trap=True, a_ho=[1.0, 1.3], Nmax=2000, Rm=1.2, dt=0.01)
    VT, WF = gpu_lib.build_tables(tcfg)
    with gpu_lib.PigsContext(tcfg, VT, WF, n_walkers=1) as ctx:
        assert ctx.L.pigs_fqt_init(ctx.h, 5, 0, 0) == ST["PIGS_ERR_UNSUPPORTED"]
        assert ctx.L.pigs_fqt_accumulate(ctx.h, 1, None) == ST["PIGS_ERR_ARG"]          # still before init
        with pytest.raises(gpu_lib.PigsError, match="periodic"):
            ctx.fqt_init(5, 0, 0)


def test_entry_points_refuse_after_a_translate_chain_time_out(gpu_lib, oracle):
    """The bounded exchange time-out of pigs_cm.hip, forced once by the test-only tuning key "cm_fault" exactly as
    tests/test_gpu_sampler.py does: afterwards the worldlines of the context are invalid, and pigs_fqt_init,
    pigs_fqt_accumulate (which never synchronises: it has to look at the flag itself) and pigs_fqt_read each return
    PIGS_ERR_HIP with the time-out's text, like every other entry point."""
    import ctypes as C
    from oracle.pyoracle import System
    cfg = SystemConfig(dim=3, Np=48, Nb=16, density=0.3, dt=5e-3, Rm=1.2, Nlev=4, Nstag=1, Lstag=8, CMFreq=1, delta_cm=0.3)
    S = System(dim=3, Np=48, Nb=16, density=0.3, dt=5e-3, Rm=1.2)
    VT, WF = gpu_lib.build_tables(cfg)
    W, Nk, Ntau, window = 3, 5, 2, 1
    ctx = gpu_lib.PigsContext(cfg, VT, WF, n_walkers=W)
    try:
        ctx.sampler_init()
        ctx.set_tuning("cm_split", 2)
        Paths = []
        for w in range(W):
            P, g = oracle.init_path(S, 700 + w)
            Paths.append(P)
            ctx.sampler_set_rng(w, g.mti, np.array(g.mt[:], np.uint32))
        ctx.upload_all(np.stack(Paths))
        ctx.fqt_init(Nk, Ntau, window)
        ctx.sampler_step(1)                       # healthy step first: everything works
        ctx.fqt_accumulate()
        healthy = ctx.fqt_read()
        assert healthy["samples"].tolist() == [1] * W and np.all(np.isfinite(healthy["F"]))
        ctx.set_tuning("cm_fault", 1)
        ctx.sampler_step(2)                       # the launch itself is asynchronous and succeeds
        with pytest.raises(gpu_lib.PigsError, match="timed out"):
            ctx.sync()
        F = np.zeros((W, Ntau + 1, Nk, 3))
        n = np.zeros(W, np.int64)
        dp, lp = C.POINTER(C.c_double), C.POINTER(C.c_int64)
        assert ctx.L.pigs_fqt_accumulate(ctx.h, W, None) == ST["PIGS_ERR_HIP"]
        assert ctx.L.pigs_fqt_read(ctx.h, F.ctypes.data_as(dp), n.ctypes.data_as(lp), None) == ST["PIGS_ERR_HIP"]
        assert ctx.L.pigs_fqt_init(ctx.h, Nk, Ntau, window) == ST["PIGS_ERR_HIP"]
        for call in (ctx.fqt_accumulate, lambda: ctx.fqt_accumulate([1]), ctx.fqt_read, lambda: ctx.fqt_read(reset=True),
                     lambda: ctx.fqt_init(Nk, Ntau, window)):
            with pytest.raises(gpu_lib.PigsError, match="timed out"):
                call()
        ctx.set_tuning("cm_fault", 0)             # the context stays invalid
        with pytest.raises(gpu_lib.PigsError, match="timed out"):
            ctx.fqt_accumulate()
    finally:
        ctx.close()


# ---- 8. non-finite coordinates ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
def test_non_finite_coordinates_stay_in_their_walker(gpu_lib, bad):
    W, Nb, Nk, window, Ntau = 4, 4, 6, 2, 3
    cfg = _cfg(3, 70, Nb)
    VT, WF = gpu_lib.build_tables(cfg)
    P = _random_paths(cfg, W, np.random.default_rng(8))
    Q = P.copy()
    Q[2, Nb + 1, 13, 1] = bad                             # walker 2, window slice Nb+1, axis 1
    with gpu_lib.PigsContext(cfg, VT, WF, n_walkers=W) as ctx:
        ctx.upload_all(P)
        ctx.fqt_init(Nk, Ntau, window)
        ctx.fqt_accumulate()
        clean = ctx.fqt_read(reset=True)["F"]
        ctx.upload_all(Q)
        ctx.fqt_accumulate()
        got = ctx.fqt_read(reset=True)
        assert got["samples"].tolist() == [1] * W
        for w in (0, 1, 3):
            assert same_bits(got["F"][w], clean[w])
        # every lag has a pair that holds slice Nb+1; only axis 1 is touched
        assert not np.isfinite(got["F"][2][:, :, 1]).any()
        assert same_bits(got["F"][2][:, :, [0, 2]], clean[2][:, :, [0, 2]])
        # the context goes on
        ctx.upload_all(P)
        ctx.fqt_accumulate()
        assert same_bits(ctx.fqt_read()["F"], clean)


# ---- 9. the front end -------------------------------------------------------------------------------------------------
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


def _tables(path, Nk, dim):
    """fqt_vpi.out -> (headers [(l, tau, n_pairs)], values [n_lags, Nk, 3*dim])."""
    hdr = []
    for ln in open(path):
        if ln.startswith("#"):
            t = ln.replace("=", " ").split()
            hdr.append((int(t[2]), float(t[4]), int(t[6])))
    a = np.loadtxt(path)
    return hdr, a.reshape(len(hdr), Nk, 3 * dim)


@pytest.mark.parametrize("ds", ["T", "F"])
def test_front_end_writes_fqt_and_changes_nothing_else(exe, tmp_path, ds):
    txt = open(os.path.join(RUNS, "he4_worm_s1982", "vpi.in")).read()
    cfg = SystemConfig.from_namelists(txt)
    off, on, w0 = str(tmp_path / "off"), str(tmp_path / "on"), str(tmp_path / "w0")
    out_off = _run(exe, txt + f"&gpu\n device_sampler = {ds}\n/\n", off)
    out = _run(exe, txt + f"&gpu\n device_sampler = {ds}, fq_tau = T, fq_ntau = 6, fq_window = 4\n/\n", on)
    assert "F(q,tau)" in out and "F(q,tau)" not in out_off
    old = _files(off)
    assert _files(on) == sorted(old + ["fqt_vpi.out"]) and "fqt_vpi.out" not in old
    for f in ("e_vpi.out", "gr_vpi.out", "sk_vpi.out", "nr_vpi.out", "worldlines_final.bin"):
        assert f in old
    for f in old:
        assert _same(off, on, f), f
    hdr, tab = _tables(os.path.join(on, "fqt_vpi.out"), cfg.Nk, cfg.dim)
    assert [h[0] for h in hdr] == list(range(7)) and [h[2] for h in hdr] == [9 - l for l in range(7)]
    assert np.allclose([h[1] for h in hdr], [l * cfg.dt for l in range(7)], rtol=1e-9)
    sk = np.loadtxt(os.path.join(on, "sk_vpi.out"))
    assert np.array_equal(tab[:, :, 0::3], np.broadcast_to(sk[:, 0::3], tab[:, :, 0::3].shape))      # the q columns
    assert np.all(np.isfinite(tab))
    # window 0: the lag-0 table is sk_vpi.out.  Both print 10 significant digits of block averages of sums that agree
    # to 1e-12*(|S|+Np)/Np per sample: after parsing they agree to that bound plus one unit of the last printed digit
    _run(exe, txt + f"&gpu\n device_sampler = {ds}, fq_tau = T\n/\n", w0)
    hdr0, tab0 = _tables(os.path.join(w0, "fqt_vpi.out"), cfg.Nk, cfg.dim)
    assert hdr0 == [(0, 0.0, 1)]
    a, b = tab0[0][:, 1::3], sk[:, 1::3]
    tol = 1e-12 * (np.abs(b) + 1.0) + 1.0000001e-9 * np.abs(b)
    worst = float(np.max(np.abs(a - b) / tol))
    print("lag-0 table against sk_vpi.out, means: worst/tol", worst)
    assert np.all(np.abs(a - b) <= tol), worst
    # the error column is sqrt((<x^2> - <x>^2)/n): a difference of the two moments, so means that agree to tol give
    # errors whose SQUARES agree to 4 |mean| tol, i.e. errors that agree to sqrt(4 |mean| tol) (|e1 - e2|^2 <= |e1^2 - e2^2|)
    ea, eb = tab0[0][:, 2::3], sk[:, 2::3]
    etol = np.sqrt(4.0 * np.abs(b) * tol) + 1.0000001e-9 * np.abs(eb)
    print("lag-0 table against sk_vpi.out, errors: worst/tol", float(np.max(np.abs(ea - eb) / etol)))
    assert np.all(np.abs(ea - eb) <= etol)


def test_front_end_sharded_contexts_one_gpu(exe, tmp_path):
    """n_walkers = 4 on two contexts of this GPU against one context: per-walker files byte-identical, the
    walker-averaged tables equal up to summation order (the block values meet in the all-reduced block vector)."""
    txt = open(os.path.join(RUNS, "he4_worm_s1982", "vpi.in")).read()
    key = "fq_tau = T, fq_ntau = 3, fq_window = 2"
    a, b = str(tmp_path / "one"), str(tmp_path / "sharded")
    _run(exe, txt + f"&gpu\n n_walkers = 4, device = 0, n_gpus = 1, {key}\n/\n", a)
    _run(exe, txt + f"&gpu\n n_walkers = 4, device = 0, n_gpus = 2, same_device = T, {key}\n/\n", b)
    for w in range(4):
        for f in ("fqt_vpi", "sk_vpi", "e_vpi"):
            assert _same(a, b, f"{f}.w{w:04d}.out"), (f, w)
    x, y = np.loadtxt(os.path.join(a, "fqt_vpi.out")), np.loadtxt(os.path.join(b, "fqt_vpi.out"))
    assert x.shape == y.shape == (4 * 50, 9) and np.all(np.isfinite(x)) and np.all(np.isfinite(y))
    # means: sums of four walkers' block values in another order (a few ulp), printed with 10 digits -> 1e-9 relative
    # after parsing (the density profiles' sharded test uses the same figure).  errors: sqrt of a difference of two
    # moments, so their squares agree to 4 |mean| * (mean's tolerance) and they to the root of that (see above).
    d = np.abs(x - y)
    mtol = 1.0000001e-9 * np.abs(x[:, 1::3])
    assert np.all(d[:, 0::3] == 0)
    assert np.all(d[:, 1::3] <= mtol)
    assert np.all(d[:, 2::3] <= np.sqrt(4.0 * np.abs(x[:, 1::3]) * mtol) + 1.0000001e-9 * np.abs(x[:, 2::3]))


def test_front_end_refuses_the_key_for_a_trapped_system(exe, tmp_path):
    txt = open(os.path.join(RUNS, "trap2d_bis_cworm0", "vpi.in")).read()
    out = _run(exe, txt + "&gpu\n fq_tau = T\n/\n", str(tmp_path), expect_rc=2)
    assert "fq_tau" in out and "periodic" in out
    assert not os.path.exists(tmp_path / "fqt_vpi.out")
