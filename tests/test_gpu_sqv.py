"""The vector structure factor S(q) on the full reciprocal grid on the MI355X (pigs_sqv_*, pigs_sqv.hip), through the
C ABI and the front end.

The expected sums come from the numpy restatement in tests/sqv_numpy.py, which forms the full phase per (vector,
particle) and does not factorise.  The bound per (walker, vector) is 1e-12 * sum over the window slices of
(|rho_q(a)|^2 + Np) with rho from the numpy side: the project's S(k) bound 1e-12*(|want| + Np)
(test_gpu_parity.py::test_structure_estimators_vs_oracle, reused by fqt_numpy.py) applied per slice.  No comparison
masks or skips elements: every (walker, vector) is compared in every case."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, ROOT
from helpers import same_bits
from pathintegralgroundstate_amd import SystemConfig
from pathintegralgroundstate_amd.profiles import normalize_sqv, shell_average
from sqv_numpy import expected, n_vectors, rho, vectors

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
    big = 16 if dim == 3 else 64
    return [(1, 0), (4, 3), (8, Nb), (big, 1)]


# ---- 1. against the numpy restatement ---------------------------------------------------------------------------------
@pytest.mark.parametrize("Nb", [4, 80])
@pytest.mark.parametrize("Np", [2, 64, 256, 257, 300, 520])
@pytest.mark.parametrize("dim", [1, 2, 3])
def test_matches_numpy_on_uploaded_worldlines(gpu_lib, dim, Np, Nb):
    W = 2
    cfg = _cfg(dim, Np, Nb)
    VT, WF = gpu_lib.build_tables(cfg)
    rng = np.random.default_rng(100000 * dim + 100 * Np + Nb)
    P = _random_paths(cfg, W, rng)
    with gpu_lib.PigsContext(cfg, VT, WF, n_walkers=W) as ctx:
        ctx.upload_all(P)
        for nmax, window in _grids(dim, Nb):
            ctx.sqv_init(nmax, window)
            n = ctx.sqv_vectors()
            assert n.shape == (((2 * nmax + 1) ** dim - 1) // 2, dim) and n.dtype == np.int32
            assert np.array_equal(n, vectors(dim, nmax))              # the restatement's own enumeration
            ctx.sqv_accumulate()
            got = ctx.sqv_read()
            A, B, cnt = expected(P, range(W), Nb, window, n, cfg.Lbox)
            assert got["S"].shape == (W, n.shape[0]) and got["samples"].dtype == np.int64
            assert np.array_equal(got["samples"], cnt)
            _assert_close(got["S"], A, B, f"dim {dim} Np {Np} Nb {Nb} nmax {nmax} W {window}")


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
    """A state evolved by a few K6 steps, accumulated every step."""
    cfg = _he4_cfg()
    W, Nb = 4, cfg.Nb
    ctx = _k6_context(gpu_lib, oracle, cfg, W)
    try:
        for nmax, window in ((4, 3), (8, Nb)):
            ctx.sqv_init(nmax, window)
            n = ctx.sqv_vectors()
            A = np.zeros((W, n.shape[0]))
            B = np.zeros_like(A)
            for istep in range(1, 4):
                ctx.sampler_step(istep)
                ctx.sqv_accumulate()
                e = expected(ctx.download_all(), range(W), Nb, window, n, cfg.Lbox)
                A, B = A + e[0], B + e[1]
            got = ctx.sqv_read()
            assert got["samples"].tolist() == [3] * W
            _assert_close(got["S"], A, B, f"sampled nmax {nmax} W {window}")
    finally:
        ctx.close()


# ---- 2. tie to the pinned estimators ------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim,Np", [(3, 64), (3, 37), (2, 300), (1, 5)])
def test_axis_vectors_are_the_pinned_structure_factor(gpu_lib, dim, Np):
    """The vectors (n,0,..), (0,n,..), .. against pigs_structure_batch summed over the window slices and against
    pigs_fqt's lag-0 table of the same window."""
    from fqt_numpy import rho as rho_axis
    W, Nb, Nk, window = 3, 6, 50, 3
    nmax = 8 if dim == 3 else 20
    cfg = _cfg(dim, Np, Nb)
    VT, WF = gpu_lib.build_tables(cfg)
    P = _random_paths(cfg, W, np.random.default_rng(dim * 1000 + Np))
    m = min(nmax, Nk)
    with gpu_lib.PigsContext(cfg, VT, WF, n_walkers=W) as ctx:
        ctx.upload_all(P)
        ctx.sqv_init(nmax, window)
        n = ctx.sqv_vectors()
        ctx.sqv_accumulate()
        got = ctx.sqv_read()["S"]
        ctx.fqt_init(Nk, 0, window)
        ctx.fqt_accumulate()
        lag0 = ctx.fqt_read()["F"][:, 0]                               # [W, Nk, dim]
        tot = np.zeros((W, Nk, dim))
        bound = np.zeros((W, Nk, dim))
        for ib in range(Nb - window, Nb + window + 1):
            tot += ctx.structure_batch(ib, cfg.Nbin, cfg.rbin, Nk)[1]
            Cc, Sn = rho_axis(P[:, ib], Nk, cfg.Lbox)
            bound += 1e-12 * ((Cc * Cc + Sn * Sn) + Np)
    axis = np.zeros((W, m, dim))
    for k in range(dim):
        for iq in range(1, m + 1):
            v = np.zeros(dim, np.int32)
            v[k] = iq
            hit = np.flatnonzero((n == v).all(axis=1))
            assert hit.size == 1
            axis[:, iq - 1, k] = got[:, hit[0]]
    _assert_close(axis, tot[:, :m], bound[:, :m], "window sum of structure_batch")
    _assert_close(axis, lag0[:, :m], bound[:, :m], "pigs_fqt lag 0")


# ---- 3. analytic: a perfect simple-cubic lattice --------------------------------------------------------------------------
@pytest.mark.parametrize("dim,m,nmax", [(3, 4, 8), (2, 16, 32)])
@pytest.mark.parametrize("shift", [0.0, 1.0 / np.sqrt(7.0)])
def test_simple_cubic_lattice(gpu_lib, dim, m, nmax, shift):
    """m^dim particles on a simple-cubic lattice, every slice identical: |rho_q|^2 = Np^2 at the stored vectors whose
    components are all multiples of m and 0 elsewhere, so a call adds Np^2 (2W+1) resp. 0 (the estimator S(q) is
    Np resp. 0); a rigid shift of the lattice by an irrational fraction of the spacing moves nothing."""
    Np, Nb, window = m ** dim, 3, 2
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
        ctx.sqv_init(nmax, window)
        n = ctx.sqv_vectors()
        ctx.sqv_accumulate()
        got = ctx.sqv_read()["S"][0]
    bragg = (n % m == 0).all(axis=1)
    assert bragg.sum() > 0 and (~bragg).sum() > 0
    ns = 2 * window + 1
    want = np.where(bragg, float(Np) * Np * ns, 0.0)
    bound = 1e-12 * ns * (np.where(bragg, float(Np) * Np, 0.0) + Np)
    _assert_close(got, want, bound, f"lattice dim {dim} shift {shift:.3f}")
    assert np.allclose(normalize_sqv(got, 1, Np, window)[bragg], Np, rtol=1e-11)


# ---- 4. determinism and independence of the launch --------------------------------------------------------------------
def test_bits_do_not_depend_on_the_launch(gpu_lib):
    W, Nb, nmax, window = 6, 5, 5, 3
    cfg = _cfg(3, 257, Nb)
    VT, WF = gpu_lib.build_tables(cfg)
    P = _random_paths(cfg, W, np.random.default_rng(5))

    def run(lists, paths=P, nw=W):
        with gpu_lib.PigsContext(cfg, VT, WF, n_walkers=nw) as ctx:
            ctx.upload_all(paths)
            ctx.sqv_init(nmax, window)
            for wl in lists:
                ctx.sqv_accumulate(wl)
            return ctx.sqv_read()

    a = run([None])
    b = run([None])                                         # a fresh context
    assert same_bits(a["S"], b["S"]) and a["samples"].tolist() == [1] * W
    assert np.all(np.isfinite(a["S"])) and np.all(a["S"] > 0)
    sub = run([[4, 1]])                                     # a subset, out of order
    assert same_bits(sub["S"][[1, 4]], a["S"][[1, 4]]) and not sub["S"][[0, 2, 3, 5]].any()
    assert sub["samples"].tolist() == [0, 1, 0, 0, 1, 0]
    twice = run([None, None])                               # two accumulates: exactly 2x
    assert same_bits(twice["S"], 2.0 * a["S"]) and twice["samples"].tolist() == [2] * W
    dup = run([[2, 0, 2, 2]])                               # listed three times: counts three times
    assert same_bits(dup["S"][2], a["S"][2] + a["S"][2] + a["S"][2]) and same_bits(dup["S"][0], a["S"][0])
    assert dup["samples"].tolist() == [1, 0, 3, 0, 0, 0]
    twice_listed = run([[3, 3]])
    assert same_bits(twice_listed["S"][3], 2.0 * a["S"][3]) and twice_listed["samples"][3] == 2
    one = run([None], paths=P[2:3], nw=1)                   # the same worldline alone in a context of one walker
    assert same_bits(one["S"][0], a["S"][2])


def test_more_than_256_walkers_in_one_list(gpu_lib):
    """A 1 024-walker context (four launches of 256 behind one call) against the same worldlines six at a time."""
    W, Nb, nmax, window = 1024, 3, 3, 2
    cfg = _cfg(2, 64, Nb)
    VT, WF = gpu_lib.build_tables(cfg)
    rng = np.random.default_rng(11)
    P6 = _random_paths(cfg, 6, rng)
    P = P6[np.arange(W) % 6]
    with gpu_lib.PigsContext(cfg, VT, WF, n_walkers=6) as ctx:
        ctx.upload_all(P6)
        ctx.sqv_init(nmax, window)
        n = ctx.sqv_vectors()
        ctx.sqv_accumulate()
        small = ctx.sqv_read()["S"]
    with gpu_lib.PigsContext(cfg, VT, WF, n_walkers=W) as ctx:
        ctx.upload_all(P)
        ctx.sqv_init(nmax, window)
        ctx.sqv_accumulate()
        big = ctx.sqv_read()
        assert big["samples"].tolist() == [1] * W
        assert same_bits(big["S"], small[np.arange(W) % 6])
        ctx.sqv_accumulate(list(range(W - 1, -1, -1)) + [7, 7, 900])      # 1 027 entries, with repeats
        big2 = ctx.sqv_read()
        cnt = np.ones(W)
        cnt[7] += 2
        cnt[900] += 1
        assert big2["samples"].tolist() == (cnt + 1).astype(int).tolist()
        want = np.stack([sum([small[w % 6]] * int(cnt[w]), big["S"][w]) for w in range(W)])
        assert same_bits(big2["S"], want)
    A, B, _ = expected(P6, range(6), Nb, window, n, cfg.Lbox)
    _assert_close(small, A, B, "1024-walker shapes")


# ---- 5. stream order and reset ------------------------------------------------------------------------------------------
def test_accumulate_sees_the_worldline_queued_before_it(gpu_lib, oracle):
    cfg = _he4_cfg()
    W, Nb, nmax, window = 4, cfg.Nb, 4, min(3, cfg.Nb)
    A = _k6_context(gpu_lib, oracle, cfg, W)
    B = _k6_context(gpu_lib, oracle, cfg, W)
    C_ = _k6_context(gpu_lib, oracle, cfg, W)
    try:
        A.sqv_init(nmax, window)
        n = A.sqv_vectors()
        A.sampler_step(1)
        A.sqv_accumulate()
        A.sampler_step(2)
        got = A.sqv_read()
        B.sampler_step(1)
        P1 = B.download_all()
        B.sqv_init(nmax, window)
        B.sqv_accumulate()
        twin = B.sqv_read()
        assert same_bits(got["S"], twin["S"])             # the twin that stopped after step 1
        E1, Bd, _ = expected(P1, range(W), Nb, window, n, cfg.Lbox)
        _assert_close(got["S"], E1, Bd, "step 1's worldline")
        B.sampler_step(2)
        P2 = B.download_all()
        E2 = expected(P2, range(W), Nb, window, n, cfg.Lbox)[0]
        assert np.any(np.abs(E2 - E1) > 10 * Bd)          # the second step moved the sums: the check has teeth
        # beside the asynchronous estimators: their results are the same bits with and without the accumulate
        C_.sqv_init(nmax, window)
        C_.sampler_step(1)
        C_.diagonal_estimators_begin(cfg.Nbin, cfg.rbin, cfg.Nk)
        C_.sqv_accumulate()
        C_.sampler_step(2)
        est = C_.diagonal_estimators_end()
        assert same_bits(C_.sqv_read()["S"], got["S"])
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


# ---- 5b. reset mask, re-init; 6. refusals -------------------------------------------------------------------------------
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
            ctx.sqv_accumulate()
        assert ctx.L.pigs_sqv_accumulate(ctx.h, 1, None) == ARG
        S1 = np.zeros(1)
        cnt = np.zeros(W, np.int64)
        nq = C.c_int64(0)
        nbuf = np.zeros(8, np.int32)
        assert ctx.L.pigs_sqv_read(ctx.h, S1.ctypes.data_as(dp), cnt.ctypes.data_as(lp), None) == ARG
        assert ctx.L.pigs_sqv_count(ctx.h, C.byref(nq)) == ARG
        assert ctx.L.pigs_sqv_vectors(ctx.h, nbuf.ctypes.data_as(ip)) == ARG
        # bad arguments (2D: nmax 1..64), and init stays undone
        for nmax, window in ((0, 0), (-2, 0), (65, 0), (5, -1), (5, Nb + 1)):
            assert ctx.L.pigs_sqv_init(ctx.h, nmax, window) == ARG, (nmax, window)
            with pytest.raises(gpu_lib.PigsError):
                ctx.sqv_init(nmax, window)
        assert ctx.L.pigs_sqv_accumulate(ctx.h, 1, None) == ARG
        # the limits themselves are accepted
        ctx.sqv_init(64, 0)
        ctx.sqv_init(1, Nb)
        ctx.sqv_init(3, 2)
        n = ctx.sqv_vectors()
        for bad in ([3], [-1], [0, 5], list(range(W)) + [W]):
            with pytest.raises(gpu_lib.PigsError):
                ctx.sqv_accumulate(bad)
        assert ctx.L.pigs_sqv_accumulate(ctx.h, -1, None) == ARG
        wl = np.array([0, W], np.int32)
        assert ctx.L.pigs_sqv_accumulate(ctx.h, 2, wl.ctypes.data_as(ip)) == ARG
        assert ctx.L.pigs_sqv_read(ctx.h, None, cnt.ctypes.data_as(lp), None) == ARG
        assert ctx.L.pigs_sqv_accumulate(ctx.h, W, None) == ST["PIGS_OK"]       # the context still works
        ctx.sqv_read(reset=True)
        assert not ctx.sqv_read()["S"].any()               # a refused list adds nothing
        # reset mask
        ctx.sqv_accumulate()
        ctx.sqv_accumulate([1])
        one = expected(P, [0, 1, 2], Nb, 2, n, cfg.Lbox)
        got = ctx.sqv_read(reset=[1, 0, 1])
        assert got["samples"].tolist() == [1, 2, 1]
        _assert_close(got["S"], one[0] * np.array([1, 2, 1.0])[:, None], one[1] * 2, "before reset")
        after = ctx.sqv_read()
        assert after["samples"].tolist() == [0, 2, 0]
        assert same_bits(after["S"][1], got["S"][1]) and not after["S"][[0, 2]].any()
        ctx.sqv_accumulate([0])
        again = ctx.sqv_read(reset=True)
        assert same_bits(again["S"][0], got["S"][0]) and again["samples"].tolist() == [1, 2, 0]
        assert not ctx.sqv_read()["S"].any() and not ctx.sqv_read()["samples"].any()
        # a second init resizes and zeroes
        ctx.sqv_accumulate()
        ctx.sqv_init(2, 1)
        z = ctx.sqv_read()
        assert z["S"].shape == (W, 12) and not z["S"].any() and not z["samples"].any()
        ctx.sqv_accumulate([2])
        e = expected(P, [2], Nb, 1, ctx.sqv_vectors(), cfg.Lbox)
        _assert_close(ctx.sqv_read()["S"], e[0], e[1], "after re-init")
    # 3D: nmax stops at 16
    cfg3 = _cfg(3, 8, 2)
    VT, WF = gpu_lib.build_tables(cfg3)
    with gpu_lib.PigsContext(cfg3, VT, WF, n_walkers=1) as ctx:
        assert ctx.L.pigs_sqv_init(ctx.h, 17, 0) == ST["PIGS_ERR_ARG"]
        ctx.sqv_init(16, 2)
        assert ctx.sqv_vectors().shape == (n_vectors(3, 16), 3)
    # 1D: nmax up to 64
    cfg1 = _cfg(1, 8, 2)
    VT, WF = gpu_lib.build_tables(cfg1)
    with gpu_lib.PigsContext(cfg1, VT, WF, n_walkers=1) as ctx:
        assert ctx.L.pigs_sqv_init(ctx.h, 65, 0) == ST["PIGS_ERR_ARG"]
        ctx.sqv_init(64, 0)
        assert ctx.sqv_vectors().ravel().tolist() == list(range(1, 65))
    # a trapped context: unsupported, a status of its own
    tcfg = SystemConfig(dim=2, Np=6, Nb=2, trap=True, a_ho=[1.0, 1.3], Nmax=2000, Rm=1.2, dt=0.01)
    VT, WF = gpu_lib.build_tables(tcfg)
    with gpu_lib.PigsContext(tcfg, VT, WF, n_walkers=1) as ctx:
        assert ctx.L.pigs_sqv_init(ctx.h, 5, 0) == ST["PIGS_ERR_UNSUPPORTED"]
        assert ctx.L.pigs_sqv_accumulate(ctx.h, 1, None) == ST["PIGS_ERR_ARG"]          # still before init
        with pytest.raises(gpu_lib.PigsError, match="periodic"):
            ctx.sqv_init(5, 0)
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


@pytest.mark.parametrize("ds", ["T", "F"])
def test_front_end_one_sample_equals_numpy(exe, tmp_path, ds):
    """One block of one step: the single sample is taken on the worldline that the run then dumps, so numpy on
    worldlines_final.bin is the whole expectation.  Bound: the kernel's, normalised, plus one unit of the last printed
    digit."""
    txt = open(os.path.join(RUNS, "he4_bis_cworm0_s1982", "vpi.in")).read()
    cfg = SystemConfig.from_namelists(txt)
    txt = re.sub(r"Nstep\s*=\s*\d+", "Nstep = 1", re.sub(r"Nblock\s*=\s*\d+", "Nblock = 1", txt))
    nmax, window = 4, 2
    d = str(tmp_path)
    out = _run(exe, txt + f"&gpu\n device_sampler = {ds}, sq_vector = T, sq_nmax = {nmax}, sq_window = {window}\n/\n", d)
    assert "Vector S(q)" in out
    P = np.fromfile(os.path.join(d, "worldlines_final.bin")).reshape((1,) + tuple(cfg.path_shape))
    n = vectors(cfg.dim, nmax)
    A, B, _ = expected(P, [0], cfg.Nb, window, n, cfg.Lbox)
    norm = (2 * window + 1) * cfg.Np
    tab = np.loadtxt(os.path.join(d, "sqvec_vpi.out"))
    assert tab.shape == (n.shape[0], cfg.dim + 3) and np.array_equal(tab[:, :cfg.dim], n)
    qb = 2 * np.pi / np.asarray(cfg.Lbox[:cfg.dim])
    assert np.allclose(tab[:, cfg.dim], np.sqrt(((n * qb) ** 2).sum(axis=1)), rtol=PRINT, atol=0)
    want = A[0] / norm
    _assert_close(tab[:, cfg.dim + 1], want, B[0] / norm + PRINT * np.abs(want), f"front end, one sample, ds {ds}")


@pytest.mark.parametrize("ds", ["T", "F"])
def test_front_end_writes_the_files_and_changes_nothing_else(exe, tmp_path, ds):
    txt = open(os.path.join(RUNS, "he4_worm_s1982", "vpi.in")).read()
    cfg = SystemConfig.from_namelists(txt)
    plain, off, on = str(tmp_path / "plain"), str(tmp_path / "off"), str(tmp_path / "on")
    out_plain = _run(exe, txt + f"&gpu\n device_sampler = {ds}\n/\n", plain)
    out_off = _run(exe, txt + f"&gpu\n device_sampler = {ds}, sq_vector = F, sq_nmax = 3\n/\n", off)
    out = _run(exe, txt + f"&gpu\n device_sampler = {ds}, sq_vector = T\n/\n", on)          # sq_nmax = 8, sq_window = 0
    assert "Vector S(q)" in out and "Vector S(q)" not in out_off and "Vector S(q)" not in out_plain
    old = _files(plain)
    assert _files(off) == old and "sqvec_vpi.out" not in old and "sq_vpi.out" not in old
    assert _files(on) == sorted(old + ["sq_vpi.out", "sqvec_vpi.out"])
    for f in old:
        assert _same(plain, off, f), f                     # key off: byte-identical to a run without it
        assert _same(plain, on, f), f                      # key on: nothing else moves
    strip = lambda s: [ln for ln in s.splitlines() if "Time per block" not in ln and "host threads" not in ln]
    assert strip(out_plain) == strip(out_off)
    dim, Nk = cfg.dim, cfg.Nk
    n = vectors(dim, 8)
    tab = np.loadtxt(os.path.join(on, "sqvec_vpi.out"))
    assert tab.shape == (n.shape[0], dim + 3) and np.array_equal(tab[:, :dim], n) and np.all(np.isfinite(tab))
    # sq_window = 0: the axis lines are sk_vpi.out.  Both print 10 digits of block averages of sums that agree to
    # 1e-12*(|S|+Np)/Np per sample: after parsing, that bound plus one unit of the last printed digit
    sk = np.loadtxt(os.path.join(on, "sk_vpi.out"))
    for k in range(dim):
        for iq in range(1, 9):
            v = np.zeros(dim)
            v[k] = iq
            row = tab[(tab[:, :dim] == v).all(axis=1)]
            assert row.shape[0] == 1
            qq, m_, e_ = sk[iq - 1, 3 * k:3 * k + 3]
            tol = 1e-12 * (abs(m_) + 1.0) + PRINT * abs(m_)
            assert abs(row[0, dim] - qq) <= PRINT * qq
            assert abs(row[0, dim + 1] - m_) <= tol, (k, iq, row[0, dim + 1], m_)
            assert abs(row[0, dim + 2] - e_) <= np.sqrt(4.0 * abs(m_) * tol) + PRINT * abs(e_)
    # sq_vpi.out is the shell average of the vector file (means of printed 10-digit values against a printed mean)
    sh = np.loadtxt(os.path.join(on, "sq_vpi.out"))
    q, mean, mult = shell_average(n, cfg.Lbox, tab[:, dim + 1])
    assert sh.shape == (q.size, 4) and np.array_equal(sh[:, 3], mult) and int(mult.sum()) == 2 * n.shape[0]
    assert np.allclose(sh[:, 0], q, rtol=PRINT, atol=0)
    assert np.all(np.abs(sh[:, 1] - mean) <= 2 * PRINT * np.abs(mean))
    assert np.all(np.isfinite(sh)) and np.all(sh[:, 2] >= 0)


def test_front_end_sharded_contexts_one_gpu(exe, tmp_path):
    """n_walkers = 4 on two contexts of this GPU against one context: per-walker files byte-identical, the
    walker-averaged files equal up to summation order (the block values meet in the all-reduced block vector, behind
    the F(q,tau) entries when both keys are on)."""
    txt = open(os.path.join(RUNS, "he4_worm_s1982", "vpi.in")).read()
    key = "fq_tau = T, fq_ntau = 2, fq_window = 1, sq_vector = T, sq_nmax = 3, sq_window = 1"
    a, b = str(tmp_path / "one"), str(tmp_path / "sharded")
    _run(exe, txt + f"&gpu\n n_walkers = 4, device = 0, n_gpus = 1, {key}\n/\n", a)
    _run(exe, txt + f"&gpu\n n_walkers = 4, device = 0, n_gpus = 2, same_device = T, {key}\n/\n", b)
    for w in range(4):
        for f in ("sqvec_vpi", "sq_vpi", "fqt_vpi", "sk_vpi", "e_vpi"):
            assert _same(a, b, f"{f}.w{w:04d}.out"), (f, w)
    # (file, rows, column of the means, column of the errors)
    for f, nrow, mean, err in (("sqvec_vpi.out", n_vectors(3, 3), [4], [5]), ("sq_vpi.out", None, [1], [2]),
                               ("fqt_vpi.out", 3 * 50, [1, 4, 7], [2, 5, 8])):
        x, y = np.loadtxt(os.path.join(a, f)), np.loadtxt(os.path.join(b, f))
        assert x.shape == y.shape and (nrow is None or x.shape[0] == nrow)
        assert np.all(np.isfinite(x)) and np.all(np.isfinite(y))
        d = np.abs(x - y)
        other = [c for c in range(x.shape[1]) if c not in mean + err]
        assert np.all(d[:, other] == 0), f                 # vectors, |q|, multiplicities
        # means: sums of four walkers' block values in another order, printed with 10 digits; errors: the root of a
        # difference of two moments (test_gpu_fqt.py has the reasoning)
        mtol = PRINT * np.abs(x[:, mean])
        assert np.all(d[:, mean] <= mtol), f
        assert np.all(d[:, err] <= np.sqrt(4.0 * np.abs(x[:, mean]) * mtol) + PRINT * np.abs(x[:, err])), f
    assert np.array_equal(np.loadtxt(os.path.join(b, "sqvec_vpi.out"))[:, :3], vectors(3, 3))


def test_front_end_refuses_the_key_for_a_trapped_system(exe, tmp_path):
    txt = open(os.path.join(RUNS, "trap2d_bis_cworm0", "vpi.in")).read()
    out = _run(exe, txt + "&gpu\n sq_vector = T\n/\n", str(tmp_path), expect_rc=2)
    assert "sq_vector" in out and "periodic" in out
    assert not os.path.exists(tmp_path / "sqvec_vpi.out")


def test_front_end_refuses_out_of_range_keys(exe, tmp_path):
    txt = open(os.path.join(RUNS, "he4_worm_s1982", "vpi.in")).read()
    for i, (extra, word) in enumerate(((", sq_nmax = 17", "sq_nmax"), (", sq_nmax = 0", "sq_nmax"),
                                       (", sq_window = 9", "sq_window"), (", sq_window = -1", "sq_window"))):
        out = _run(exe, txt + f"&gpu\n sq_vector = T{extra}\n/\n", str(tmp_path / str(i)), expect_rc=2)
        assert "sq_vector" in out and word in out
        assert not os.path.exists(tmp_path / str(i) / "e_vpi.out")
