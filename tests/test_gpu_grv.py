"""The pair distribution on the vector grid over a slice window on the MI355X (pigs_grv_*, pigs_grv.hip), through the
C ABI and the front end.

The expected counts come from the numpy restatement in tests/grv_numpy.py.  Everything is an integer count, so every
comparison is exact equality over all elements: nothing is masked or skipped.  Every case runs with the vector grid in
global memory (grv_form 0), privatised in LDS (grv_form 1) where the grid fits, and with the automatic choice."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, ROOT
from grv_numpy import Window
from pathintegralgroundstate_amd import SystemConfig

pytestmark = pytest.mark.gpu
RUNS = os.path.join(GOLDEN, "vpi_runs")
HOST = os.path.join(ROOT, "pathintegralgroundstate_amd", "host")
DENSITY = {1: 0.2, 2: 0.25, 3: 0.365}
NBMAX = {1: 4096, 2: 1024, 3: 128}


def _header():
    return open(os.path.join(ROOT, "include", "pigs_hip.h")).read()


def _status_codes():
    return {k: int(v) for k, v in re.findall(r"^\s*(PIGS_\w+)\s*=\s*(-?\d+)", _header(), flags=re.M)}


def _constant(name):
    txt = open(os.path.join(ROOT, "pathintegralgroundstate_amd", "csrc", "pigs_kernels.h")).read()
    return int(re.search(r"constexpr\s+\w+\s+" + name + r"\s*=\s*(\d+)\s*;", txt).group(1))


ST = _status_codes()
assert ST["PIGS_OK"] == 0 and len({ST["PIGS_ERR_ARG"], ST["PIGS_ERR_HIP"], ST["PIGS_ERR_UNSUPPORTED"]}) == 3
LDS_BINS = _constant("kDensLdsBins")
TILE = _constant("kGrvTile")
LDS_BUDGET = 160 * 1024


def _cfg(dim, Np, Nb, **kw):
    return SystemConfig(dim=dim, Np=Np, Nb=Nb, density=DENSITY[dim], **kw)


def _random_paths(cfg, W, rng, scale=0.5):
    L = np.asarray(cfg.Lbox[:cfg.dim])
    return rng.uniform(-scale, scale, (W,) + tuple(cfg.path_shape)) * L


def _rbin(cfg, Nr):
    return cfg.rcut / float(np.float32(Nr))


def _fits(dim, Nbin, Nr):
    """The LDS form's footprint: two staging tiles, the radial histogram where it is privatised, the u32 grid."""
    return 2 * dim * TILE * 8 + (4 * Nr if Nr <= LDS_BINS else 0) + 4 * Nbin ** dim <= LDS_BUDGET


def _forms(gpu_lib, ctx, dim, Nbin, Nr, init):
    """The forms to run: sets the tuning key, calls init() and yields; a forced LDS form that does not fit must be
    refused instead."""
    for form in (0, 1, -1):
        ctx.set_tuning("grv_form", form)
        init()
        if form == 1 and not _fits(dim, Nbin, Nr):
            assert ctx.L.pigs_grv_accumulate(ctx.h, 1, None) == ST["PIGS_ERR_ARG"]
            with pytest.raises(gpu_lib.PigsError, match="LDS"):
                ctx.grv_accumulate()
            continue
        yield form
    ctx.set_tuning("grv_form", -1)


def _check(got, V, R, cnt, what):
    assert got["vec"].shape == V.shape and got["vec"].dtype == np.int64, (what, got["vec"].shape, V.shape)
    assert got["radial"].shape == R.shape and got["radial"].dtype == np.int64 and got["samples"].dtype == np.int64
    assert np.array_equal(got["samples"], cnt), (what, got["samples"], cnt)
    nv = int(np.count_nonzero(got["vec"] != V))
    nr = int(np.count_nonzero(got["radial"] != R))
    print(f"{what}: vec {got['vec'].sum()} counts, {nv} bins differ; radial {got['radial'].sum()} counts, {nr} bins differ")
    assert nv == 0 and nr == 0, what


# ---- 1. against the numpy restatement on random in-box worldlines ------------------------------------------------------
@pytest.mark.parametrize("Nb", [4, 20])
@pytest.mark.parametrize("Np", [2, 3, 64, 65, 256, 257, 300, 520])
@pytest.mark.parametrize("dim", [1, 2, 3])
def test_matches_numpy_on_uploaded_worldlines(gpu_lib, dim, Np, Nb):
    W = 2
    cfg = _cfg(dim, Np, Nb)
    VT, WF = gpu_lib.build_tables(cfg)
    P = _random_paths(cfg, W, np.random.default_rng(100000 * dim + 100 * Np + Nb))
    pairs = Np * (Np - 1) // 2
    with gpu_lib.PigsContext(cfg, VT, WF, n_walkers=W) as ctx:
        ctx.upload_all(P)
        # (the largest grid: the per-dimension limit, 2 walkers x 128^3 x 8 B = 32 MiB at most, far inside 2 GiB)
        for Nbin, window in ((1, 0), (4, 3), (16, Nb), (NBMAX[dim], 1)):
            ref = Window(P, Nb, window, cfg.Lbox, cfg.rcut2)
            for Nr in (1, 50, LDS_BINS + 1):
                rbin = _rbin(cfg, Nr)
                V, R, cnt, dropped = ref.expected(range(W), Nbin, Nr, rbin)
                assert dropped == 0                                    # in-box worldlines: no pair leaves the cell
                for form in _forms(gpu_lib, ctx, dim, Nbin, Nr, lambda: ctx.grv_init(Nbin, window, Nr, rbin)):
                    ctx.grv_accumulate()
                    got = ctx.grv_read()
                    # the cap first: a dropping bug cannot hide
                    tot = got["vec"].reshape(W, -1).sum(axis=1)
                    assert np.array_equal(tot, got["samples"] * (2 * window + 1) * pairs), (form, Nbin, window, tot)
                    _check(got, V, R, cnt, f"dim {dim} Np {Np} Nb {Nb} Nbin {Nbin} W {window} Nr {Nr} form {form}")


# ---- 2. inputs that must be dropped or sit on edges -----------------------------------------------------------------------
def _edge_paths(cfg, kind, rng, window):
    L = np.asarray(cfg.Lbox[:cfg.dim])
    Nb = cfg.Nb
    if kind == "outside":                                   # differences pass 1.5 L: one fold leaves them outside
        return _random_paths(cfg, 2, rng, scale=1.3)
    P = _random_paths(cfg, 2, rng)
    if kind == "coincident":                                # d = 0: t = Nbin/2 exactly
        P[:, :, 1] = P[:, :, 0]
    elif kind == "half_box":                                # d = +L/2 on axis 0 (walker 0) and -L/2 (walker 1), exactly
        P[0, :, 0, 0], P[0, :, 1, 0] = 0.25 * L[0], -0.25 * L[0]
        P[1, :, 0, 0], P[1, :, 1, 0] = -0.25 * L[0], 0.25 * L[0]
        P[:, :, 1, 1:] = P[:, :, 0, 1:]
    elif kind == "nonfinite":                               # in a window slice and in a slice outside the window
        for a, v in ((Nb, np.nan), (Nb - window, np.inf), (Nb + window, 1e300), (0, np.nan), (2 * Nb, np.inf)):
            P[0, a, 1] = v
            P[1, a, 0, 0] = v
    return P


@pytest.mark.parametrize("kind", ["outside", "coincident", "half_box", "nonfinite"])
@pytest.mark.parametrize("dim,Np", [(1, 5), (2, 70), (3, 257)])
def test_dropped_and_edge_inputs_equal_numpy(gpu_lib, dim, Np, kind):
    Nb, window, W = 5, 2, 2
    cfg = _cfg(dim, Np, Nb)
    VT, WF = gpu_lib.build_tables(cfg)
    P = _edge_paths(cfg, kind, np.random.default_rng(7 * dim + Np), window)
    ref = Window(P, Nb, window, cfg.Lbox, cfg.rcut2)
    with gpu_lib.PigsContext(cfg, VT, WF, n_walkers=W) as ctx:
        ctx.upload_all(P)
        for Nbin, Nr in ((4, 50), (7, 1), (16, LDS_BINS + 1)):
            rbin = _rbin(cfg, Nr)
            V, R, cnt, dropped = ref.expected(range(W), Nbin, Nr, rbin)
            if kind in ("outside", "nonfinite"):
                assert dropped > 0                                     # the inputs do what they are here for
            for form in _forms(gpu_lib, ctx, dim, Nbin, Nr, lambda: ctx.grv_init(Nbin, window, Nr, rbin)):
                ctx.grv_accumulate()
                got = ctx.grv_read()
                _check(got, V, R, cnt, f"{kind} dim {dim} Np {Np} Nbin {Nbin} Nr {Nr} form {form}")
                pairs = (2 * window + 1) * Np * (Np - 1) // 2
                assert np.all(got["vec"].reshape(W, -1).sum(axis=1) <= pairs)


# ---- 3. tie to the pinned estimator --------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim,Np", [(3, 64), (3, 37), (2, 300), (1, 5)])
def test_radial_is_the_pinned_pair_correlation(gpu_lib, dim, Np):
    """2 * radial equals pigs_structure_batch's gr summed over the window slices, exactly."""
    W, Nb, window, Nr = 3, 6, 3, 50
    cfg = _cfg(dim, Np, Nb)
    VT, WF = gpu_lib.build_tables(cfg)
    P = _random_paths(cfg, W, np.random.default_rng(dim * 1000 + Np))
    rbin = _rbin(cfg, Nr)
    with gpu_lib.PigsContext(cfg, VT, WF, n_walkers=W) as ctx:
        ctx.upload_all(P)
        tot = np.zeros((W, Nr))
        for ib in range(Nb - window, Nb + window + 1):
            tot += ctx.structure_batch(ib, Nr, rbin, 1)[0]
        assert tot.sum() > 0
        for form in _forms(gpu_lib, ctx, dim, 8, Nr, lambda: ctx.grv_init(8, window, Nr, rbin)):
            ctx.grv_accumulate()
            got = ctx.grv_read()
            assert np.array_equal(2 * got["radial"], tot.astype(np.int64)) and np.array_equal(tot, np.rint(tot)), form


# ---- 4. semantics ------------------------------------------------------------------------------------------------------
def test_lists_repeats_resets_and_reinit(gpu_lib):
    W, Nb, window, Nbin, Nr = 6, 5, 2, 5, 20
    cfg = _cfg(3, 257, Nb)
    VT, WF = gpu_lib.build_tables(cfg)
    P = _random_paths(cfg, W, np.random.default_rng(5))
    ref = Window(P, Nb, window, cfg.Lbox, cfg.rcut2)
    rbin = _rbin(cfg, Nr)
    with gpu_lib.PigsContext(cfg, VT, WF, n_walkers=W) as ctx:
        ctx.upload_all(P)
        for form in _forms(gpu_lib, ctx, 3, Nbin, Nr, lambda: ctx.grv_init(Nbin, window, Nr, rbin)):
            # a subset out of order, one walker listed three times; the unlisted ones stay exactly zero
            wl = [4, 1, 2, 2, 2]
            ctx.grv_accumulate(wl)
            got = ctx.grv_read()
            _check(got, *ref.expected(wl, Nbin, Nr, rbin)[:3], f"list form {form}")
            assert got["samples"].tolist() == [0, 1, 3, 0, 1, 0]
            assert not got["vec"][[0, 3, 5]].any() and not got["radial"][[0, 3, 5]].any()
            assert np.array_equal(got["vec"][2], 3 * ref.expected([2], Nbin, Nr, rbin)[0][2])
            # per-walker reset mask
            keep = ctx.grv_read(reset=[0, 1, 1, 0, 0, 1])
            _check(keep, got["vec"], got["radial"], got["samples"], "read with a mask returns the counts first")
            after = ctx.grv_read()
            assert after["samples"].tolist() == [0, 0, 0, 0, 1, 0]
            assert np.array_equal(after["vec"][4], got["vec"][4]) and not after["vec"][[0, 1, 2, 3, 5]].any()
            assert np.array_equal(after["radial"][4], got["radial"][4]) and not after["radial"][[0, 1, 2, 3, 5]].any()
            # one list of all walkers against one call per walker
            ctx.grv_read(reset=True)
            z = ctx.grv_read()
            assert not z["vec"].any() and not z["radial"].any() and not z["samples"].any()
            ctx.grv_accumulate()
            whole = ctx.grv_read(reset=True)
            for w in range(W):
                ctx.grv_accumulate([w])
            single = ctx.grv_read(reset=True)
            _check(single, whole["vec"], whole["radial"], whole["samples"], "one call per walker")
            _check(whole, *ref.expected(range(W), Nbin, Nr, rbin)[:3], f"all walkers form {form}")
            # a second init with another Nbin resizes and zeroes
            ctx.grv_accumulate()
            ctx.grv_init(Nbin + 2, 1, Nr, rbin)
            z = ctx.grv_read()
            assert z["vec"].shape == (W,) + (Nbin + 2,) * 3 and not z["vec"].any() and not z["radial"].any()
            assert not z["samples"].any()
            ctx.grv_accumulate([3])
            ref1 = Window(P, Nb, 1, cfg.Lbox, cfg.rcut2)
            _check(ctx.grv_read(), *ref1.expected([3], Nbin + 2, Nr, rbin)[:3], "after re-init")


def test_three_hundred_walkers_at_two_particles(gpu_lib):
    """Np = 2 and a list of 300 walkers (two launches), then a longer list with repeats."""
    W, Nb, window, Nbin, Nr = 300, 3, 2, 6, 10
    cfg = _cfg(2, 2, Nb)
    VT, WF = gpu_lib.build_tables(cfg)
    P = _random_paths(cfg, W, np.random.default_rng(11))
    ref = Window(P, Nb, window, cfg.Lbox, cfg.rcut2)
    rbin = _rbin(cfg, Nr)
    with gpu_lib.PigsContext(cfg, VT, WF, n_walkers=W) as ctx:
        ctx.upload_all(P)
        for form in _forms(gpu_lib, ctx, 2, Nbin, Nr, lambda: ctx.grv_init(Nbin, window, Nr, rbin)):
            ctx.grv_accumulate()
            got = ctx.grv_read(reset=True)
            V, R, cnt, dropped = ref.expected(range(W), Nbin, Nr, rbin)
            assert dropped == 0
            _check(got, V, R, cnt, f"300 walkers form {form}")
            assert np.array_equal(got["vec"].reshape(W, -1).sum(axis=1), np.full(W, 2 * window + 1))
            wl = list(range(W - 1, -1, -1)) + [7, 7, 299]
            ctx.grv_accumulate(wl)
            _check(ctx.grv_read(), *ref.expected(wl, Nbin, Nr, rbin)[:3], f"303 entries form {form}")


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


def test_accumulate_queued_behind_the_sampler_step(gpu_lib, oracle):
    """Three K6 steps, each followed at once by an accumulate, with no synchronisation in between: the counts are
    numpy's on the worldlines of those three steps (a twin context downloads them)."""
    cfg = SystemConfig.from_namelists(open(os.path.join(RUNS, "he4_bis_cworm0_s1982", "vpi.in")).read())
    W, Nb, Nbin, Nr = 4, cfg.Nb, 8, cfg.Nbin
    window = min(3, Nb)
    rbin = _rbin(cfg, Nr)
    for form in (0, 1, -1):
        A = _k6_context(gpu_lib, oracle, cfg, W)
        B = _k6_context(gpu_lib, oracle, cfg, W)
        try:
            A.set_tuning("grv_form", form)
            A.grv_init(Nbin, window)                        # the defaults: Nr = the context's Nbin, rbin = rcut/float32(Nbin)
            for istep in range(1, 4):
                A.sampler_step(istep)
                A.grv_accumulate()
            got = A.grv_read()
            final = A.download_all()
            V = np.zeros_like(got["vec"])
            R = np.zeros_like(got["radial"])
            moved = []
            for istep in range(1, 4):
                B.sampler_step(istep)
                Pn = B.download_all()
                e = Window(Pn, Nb, window, cfg.Lbox, cfg.rcut2).expected(range(W), Nbin, Nr, rbin)
                V, R = V + e[0], R + e[1]
                moved.append(e[0])
            assert np.array_equal(final, Pn)                # the twin followed the same worldlines
            assert np.any(moved[0] != moved[2])             # the steps moved the counts: the check has teeth
            _check(got, V, R, np.full(W, 3), f"behind sampler_step form {form}")
        finally:
            A.close()
            B.close()


# ---- 5. status codes -----------------------------------------------------------------------------------------------------
def test_status_codes(gpu_lib):
    W, Nb = 3, 4
    cfg = _cfg(2, 40, Nb)
    VT, WF = gpu_lib.build_tables(cfg)
    P = _random_paths(cfg, W, np.random.default_rng(3))
    lp, ip = C.POINTER(C.c_int64), C.POINTER(C.c_int32)
    ARG, OK = ST["PIGS_ERR_ARG"], ST["PIGS_OK"]
    buf = np.zeros(64, np.int64)
    b = buf.ctypes.data_as(lp)
    with gpu_lib.PigsContext(cfg, VT, WF, n_walkers=W) as ctx:
        ctx.upload_all(P)
        # before init
        with pytest.raises(gpu_lib.PigsError):
            ctx.grv_accumulate()
        with pytest.raises(gpu_lib.PigsError):
            ctx.grv_read()
        assert ctx.L.pigs_grv_accumulate(ctx.h, 1, None) == ARG
        assert ctx.L.pigs_grv_read(ctx.h, b, b, b, None) == ARG
        # bad arguments (2D: Nbin 1..1024), and init stays undone
        for Nbin, Nr, rbin, window in ((0, 5, 0.1, 0), (-3, 5, 0.1, 0), (1025, 5, 0.1, 0), (4, 0, 0.1, 0), (4, -1, 0.1, 0),
                                       (4, 5, 0.0, 0), (4, 5, -0.1, 0), (4, 5, float("nan"), 0), (4, 5, float("inf"), 0),
                                       (4, 5, 0.1, -1), (4, 5, 0.1, Nb + 1)):
            assert ctx.L.pigs_grv_init(ctx.h, Nbin, Nr, rbin, window) == ARG, (Nbin, Nr, rbin, window)
            with pytest.raises(gpu_lib.PigsError):
                ctx.grv_init(Nbin, window, Nr, rbin)
        assert ctx.L.pigs_grv_accumulate(ctx.h, 1, None) == ARG
        # 2 GiB: 3 walkers x (16 + Nr + 1) x 8 B
        assert ctx.L.pigs_grv_init(ctx.h, 4, 2 ** 27, 0.1, 0) == ARG
        assert ctx.L.pigs_grv_init(ctx.h, 1024, 2 ** 27, 0.1, 0) == ARG
        # the limits themselves are accepted
        ctx.grv_init(1024, Nb, 1, 1e-300)
        ctx.grv_init(1, 0)
        ctx.grv_init(3, 2, 7, 0.3)
        for bad in ([3], [-1], [0, 5], list(range(W)) + [W]):
            with pytest.raises(gpu_lib.PigsError):
                ctx.grv_accumulate(bad)
        assert ctx.L.pigs_grv_accumulate(ctx.h, -1, None) == ARG
        wl = np.array([0, W], np.int32)
        assert ctx.L.pigs_grv_accumulate(ctx.h, 2, wl.ctypes.data_as(ip)) == ARG
        assert ctx.L.pigs_grv_read(ctx.h, None, b, b, None) == ARG
        assert ctx.L.pigs_set_tuning(ctx.h, b"grv_form", 2) == ARG and ctx.L.pigs_set_tuning(ctx.h, b"grv_form", -2) == ARG
        assert ctx.L.pigs_grv_accumulate(ctx.h, W, None) == OK          # the context still works
        got = ctx.grv_read(reset=True)
        assert got["samples"].tolist() == [1] * W                       # the refused lists added nothing
        _check(got, *Window(P, Nb, 2, cfg.Lbox, cfg.rcut2).expected(range(W), 3, 7, 0.3)[:3], "after the refusals")
        # a forced LDS form whose grid does not fit is refused at the accumulate, and adds nothing
        ctx.grv_init(1024, 0)
        ctx.set_tuning("grv_form", 1)
        assert ctx.L.pigs_grv_accumulate(ctx.h, W, None) == ARG
        ctx.set_tuning("grv_form", -1)
        z = ctx.grv_read()
        assert not z["vec"].any() and not z["samples"].any()
        ctx.grv_accumulate()
        assert ctx.grv_read()["samples"].tolist() == [1] * W
    for dim, lim in NBMAX.items():
        c = _cfg(dim, 8, 2)
        VT, WF = gpu_lib.build_tables(c)
        with gpu_lib.PigsContext(c, VT, WF, n_walkers=1) as ctx:
            assert ctx.L.pigs_grv_init(ctx.h, lim + 1, 5, 0.1, 0) == ARG
            ctx.grv_init(lim, 2)
            assert ctx.grv_read()["vec"].shape == (1,) + (lim,) * dim
    # a trapped context: unsupported, a status of its own
    tcfg = SystemConfig(dim=2, Np=6, Nb=2, trap=True, a_ho=[1.0, 1.3], Nmax=2000, Rm=1.2, dt=0.01)
    VT, WF = gpu_lib.build_tables(tcfg)
    with gpu_lib.PigsContext(tcfg, VT, WF, n_walkers=1) as ctx:
        assert ctx.L.pigs_grv_init(ctx.h, 5, 5, 0.1, 0) == ST["PIGS_ERR_UNSUPPORTED"]
        assert ctx.L.pigs_grv_accumulate(ctx.h, 1, None) == ARG         # still before init
        with pytest.raises(gpu_lib.PigsError, match="periodic"):
            ctx.grv_init(5, 0, 5, 0.1)
        ctx.sync()                                                      # the context still works


# ---- 6. the front end -------------------------------------------------------------------------------------------------
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


def test_front_end_writes_the_files_and_changes_nothing_else(exe, tmp_path):
    txt = open(os.path.join(RUNS, "he4_worm_s1982", "vpi.in")).read()
    cfg = SystemConfig.from_namelists(txt)
    plain, on = str(tmp_path / "plain"), str(tmp_path / "on")
    out_plain = _run(exe, txt, plain)
    Ng = 6
    out = _run(exe, txt + f"&gpu\n gr_vector = T, gr_nbin = {Ng}, gr_window = 0\n/\n", on)
    assert "Vector g(r)" in out and "Vector g(r)" not in out_plain
    old = _files(plain)
    assert "grvec_vpi.out" not in old and "grw_vpi.out" not in old
    assert _files(on) == sorted(old + ["grvec_vpi.out", "grw_vpi.out"])
    for f in old:
        assert _same(plain, on, f), f                      # nothing else moves
    # gr_window = 0: every mean of grw_vpi.out is gr_vpi.out's, to the printed digits
    gw, gr = np.loadtxt(os.path.join(on, "grw_vpi.out")), np.loadtxt(os.path.join(on, "gr_vpi.out"))
    assert gw.shape == gr.shape == (cfg.Nbin, 3) and gr[:, 1].max() > 0.5
    assert np.array_equal(gw[:, 0], gr[:, 0]) and np.array_equal(gw[:, 1], gr[:, 1])
    # grvec_vpi.out: Nbin^dim lines at the bin centres in flat-index order (x fastest), inversion-symmetric
    dim = cfg.dim
    tab = np.loadtxt(os.path.join(on, "grvec_vpi.out"))
    assert tab.shape == (Ng ** dim, dim + 2) and np.all(np.isfinite(tab)) and tab[:, dim].max() > 0
    j = np.arange(Ng ** dim)
    for k in range(dim):
        b = cfg.Lbox[k] / Ng
        want = -0.5 * cfg.Lbox[k] + ((j // Ng ** k) % Ng + 0.5) * b
        assert np.allclose(tab[:, k], want, rtol=PRINT, atol=PRINT * cfg.Lbox[k])
    assert np.array_equal(tab[:, dim], tab[::-1, dim]) and np.array_equal(tab[:, dim + 1], tab[::-1, dim + 1])
    # the sum rule: the grid mean is 1 - 1/Np less the pairs that one fold left outside the cell (10 printed digits)
    assert 0 < tab[:, dim].mean() <= (1.0 - 1.0 / cfg.Np) * (1 + 2 * PRINT)
    print("grid mean of g", tab[:, dim].mean(), "ideal", 1.0 - 1.0 / cfg.Np)


def test_front_end_sharded_contexts_one_gpu(exe, tmp_path):
    """n_walkers = 4 on two contexts of this GPU against one context: the two files agree to one unit of the last
    printed digit (the block values meet in the all-reduced block vector in another order)."""
    txt = open(os.path.join(RUNS, "he4_worm_s1982", "vpi.in")).read()
    key = "gr_vector = T, gr_nbin = 5, gr_window = 2"
    a, b = str(tmp_path / "one"), str(tmp_path / "sharded")
    _run(exe, txt + f"&gpu\n n_walkers = 4, device = 0, n_gpus = 1, {key}\n/\n", a)
    _run(exe, txt + f"&gpu\n n_walkers = 4, device = 0, n_gpus = 2, same_device = T, {key}\n/\n", b)
    for w in range(4):
        for f in ("grvec_vpi", "grw_vpi", "gr_vpi", "e_vpi"):
            assert _same(a, b, f"{f}.w{w:04d}.out"), (f, w)
    for f, nrow, ncoord in (("grvec_vpi.out", 125, 3), ("grw_vpi.out", 100, 1)):
        x, y = np.loadtxt(os.path.join(a, f)), np.loadtxt(os.path.join(b, f))
        assert x.shape == y.shape == (nrow, ncoord + 2) and np.all(np.isfinite(x)) and np.all(np.isfinite(y))
        assert np.array_equal(x[:, :ncoord], y[:, :ncoord])
        mean, err = x[:, ncoord], x[:, ncoord + 1]
        mtol = PRINT * np.abs(mean)
        assert np.all(np.abs(mean - y[:, ncoord]) <= mtol), f
        # errors: the root of a difference of two moments (test_gpu_fqt.py has the reasoning)
        assert np.all(np.abs(err - y[:, ncoord + 1]) <= np.sqrt(4.0 * np.abs(mean) * mtol) + PRINT * np.abs(err)), f


def test_front_end_refusals(exe, tmp_path):
    txt = open(os.path.join(RUNS, "trap2d_bis_cworm0", "vpi.in")).read()
    out = _run(exe, txt + "&gpu\n gr_vector = T\n/\n", str(tmp_path / "trap"), expect_rc=2)
    assert "gr_vector" in out and "periodic" in out
    txt = open(os.path.join(RUNS, "he4_worm_s1982", "vpi.in")).read()
    for i, (extra, word) in enumerate(((", gr_nbin = 129", "gr_nbin"), (", gr_nbin = 0", "gr_nbin"),
                                       (", gr_window = 9", "gr_window"), (", gr_window = -1", "gr_window"))):
        out = _run(exe, txt + f"&gpu\n gr_vector = T{extra}\n/\n", str(tmp_path / str(i)), expect_rc=2)
        assert "gr_vector" in out and word in out
        assert not os.path.exists(tmp_path / str(i) / "e_vpi.out")
