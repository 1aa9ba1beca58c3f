"""Density profiles and pair distribution of a trapped system on the MI355X (pigs_density_*, pigs_density.hip).

The expected counts come from a numpy restatement of the definitions in include/pigs_hip.h, with the same expressions in
the same order; counts are 64-bit integers, so every comparison is exact (np.array_equal)."""
import os
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, ROOT
from pathintegralgroundstate_amd import SystemConfig

pytestmark = pytest.mark.gpu
RUNS = os.path.join(GOLDEN, "vpi_runs")
HOST = os.path.join(ROOT, "pathintegralgroundstate_amd", "host")
KEY = "density_profile = T"
NEW_FILES = ("dens_vpi.out", "rho_vpi.out", "pr_vpi.out")


# ---- numpy restatement -----------------------------------------------------------------------------------------------
def ref_counts(R, Nbin, h):
    """planar, radial, pair counts of one slice R[Np, dim] (planar flat, x fastest)."""
    b = (2.0 * h) / Nbin
    br = h / Nbin
    Np, dim = R.shape
    dp = min(dim, 2)
    planar = np.zeros(Nbin ** dp, np.int64)
    radial = np.zeros(Nbin, np.int64)
    pair = np.zeros(Nbin, np.int64)
    with np.errstate(all="ignore"):
        t = (R[:, :dp] + h) / b
        ok = np.all((t >= 0.0) & (t < Nbin), axis=1)
        j = np.where(ok[:, None], t, 0.0).astype(np.int64)
        flat = j[:, 0] + (Nbin * j[:, 1] if dp == 2 else 0)
        np.add.at(planar, flat[ok], 1)
        r2 = R[:, 0] * R[:, 0]
        for k in range(1, dim):
            r2 = r2 + R[:, k] * R[:, k]
        u = np.sqrt(r2) / br
        ok = u < Nbin
        np.add.at(radial, u[ok].astype(np.int64), 1)
        i, jj = np.triu_indices(Np, 1)
        d = R[i] - R[jj]
        d2 = d[:, 0] * d[:, 0]
        for k in range(1, dim):
            d2 = d2 + d[:, k] * d[:, k]
        u = np.sqrt(d2) / br
        ok = u < Nbin
        np.add.at(pair, u[ok].astype(np.int64), 2)
    return planar, radial, pair


def expected(slices, walkers, Nbin, h, W):
    """Accumulated counts of the walker list `walkers` (entries may repeat) over slices[W, Np, dim]."""
    dim = slices.shape[2]
    dp = min(dim, 2)
    out = {"planar": np.zeros((W, Nbin ** dp), np.int64), "radial": np.zeros((W, Nbin), np.int64),
           "pair": np.zeros((W, Nbin), np.int64), "samples": np.zeros(W, np.int64)}
    for w in walkers:
        p, r, q = ref_counts(slices[w], Nbin, h)
        out["planar"][w] += p
        out["radial"][w] += r
        out["pair"][w] += q
        out["samples"][w] += 1
    out["planar"] = out["planar"].reshape((W,) + (Nbin,) * dp)
    return out


def assert_counts(got, want):
    for k in ("planar", "radial", "pair", "samples"):
        assert got[k].dtype == np.int64 and got[k].shape == want[k].shape, (k, got[k].shape, want[k].shape)
        assert np.array_equal(got[k], want[k]), k


def _trap_cfg(dim, Np, Nb=2):
    return SystemConfig(dim=dim, Np=Np, Nb=Nb, trap=True, a_ho=[1.0, 1.3, 0.8], Nmax=2000, Rm=1.2, dt=0.01)


def _worldlines(cfg, W, h, Nbin, rng, specials=True):
    """Gaussian cloud of width ~h/2 (some particles beyond the grid) with, on slice Nb, particles placed on bin edges,
    far outside, at +-Inf, NaN and +-1e300."""
    P = rng.normal(0.0, 0.5 * h, (W,) + cfg.path_shape)
    if specials:
        b = (2.0 * h) / Nbin
        edges = np.array([-h + j * b for j in range(Nbin + 1)] + [-h, h, h / Nbin, 2.0 * h / Nbin])
        odd = np.array([50.0 * h, -50.0 * h, np.inf, -np.inf, np.nan, 1e300, -1e300, 0.0])
        vals = np.concatenate([edges, odd])
        S = P[:, cfg.Nb]
        for w in range(W):
            n = min(cfg.Np - 1, len(vals))
            idx = rng.choice(cfg.Np, n, replace=False)
            for c, ip in enumerate(idx):
                k = c % cfg.dim
                S[w, ip, k] = vals[(c + w) % len(vals)]
                if c % 3 == 0:
                    S[w, ip, :] = vals[(c + w) % len(vals)]      # all coordinates on the same edge / special value
    return P


@pytest.mark.parametrize("dim,Np", [(d, n) for d in (1, 2, 3) for n in (2, 65, 300)] + [(2, 1100)])
def test_kernel_matches_numpy(gpu_lib, dim, Np):
    """Uploaded trapped worldlines; Nbin 1, 7, 100 (re-init on the same context); walker lists: all, a subset, one with a
    duplicate.  Np = 1100 takes the tiled pair loop (more than one LDS tile of partners)."""
    W, h = 3, 1.5
    cfg = _trap_cfg(dim, Np)
    VT, WF = gpu_lib.build_tables(cfg)
    rng = np.random.default_rng(1000 * dim + Np)
    with gpu_lib.PigsContext(cfg, VT, WF, n_walkers=W) as ctx:
        for Nbin in (1, 7, 100):
            P = _worldlines(cfg, W, h, Nbin, rng)
            ctx.upload_all(P)
            slices = P[:, cfg.Nb]
            ctx.density_init(Nbin, h)
            for walkers in (None, [2, 0], [1, 1, 2]):
                ctx.density_accumulate(walkers)
                got = ctx.density_read(reset=True)
                assert_counts(got, expected(slices, range(W) if walkers is None else walkers, Nbin, h, W))


def test_kernel_global_atomic_pair_form(gpu_lib):
    """Nbin beyond the LDS pair histogram (kDensLdsBins = 8192 in pigs_kernels.h): the pair counts go straight to
    global memory with 64-bit atomics."""
    W, h, Nbin = 3, 1.5, 9000
    cfg = _trap_cfg(1, 300)
    VT, WF = gpu_lib.build_tables(cfg)
    rng = np.random.default_rng(7)
    P = _worldlines(cfg, W, h, Nbin, rng)
    P[:, cfg.Nb, :40, 0] = P[:, cfg.Nb, 40:80, 0]      # coinciding particles: many pairs in bin 0
    with gpu_lib.PigsContext(cfg, VT, WF, n_walkers=W) as ctx:
        ctx.upload_all(P)
        ctx.density_init(Nbin, h)
        ctx.density_accumulate([0, 2, 2])
        assert_counts(ctx.density_read(), expected(P[:, cfg.Nb], [0, 2, 2], Nbin, h, W))


def test_accumulator_semantics(gpu_lib):
    W, h, Nbin = 3, 2.0, 11
    cfg = _trap_cfg(2, 40)
    VT, WF = gpu_lib.build_tables(cfg)
    rng = np.random.default_rng(3)
    P = _worldlines(cfg, W, h, Nbin, rng, specials=False)
    S = P[:, cfg.Nb]
    with gpu_lib.PigsContext(cfg, VT, WF, n_walkers=W) as ctx:
        ctx.upload_all(P)
        with pytest.raises(gpu_lib.PigsError):
            ctx.density_accumulate()                       # before density_init
        assert ctx.L.pigs_density_accumulate(ctx.h, 1, None) != 0
        ctx.density_init(Nbin, h)
        # two accumulates add up
        ctx.density_accumulate()
        ctx.density_accumulate([0, 1, 2])
        assert_counts(ctx.density_read(), expected(S, [0, 1, 2, 0, 1, 2], Nbin, h, W))
        # a per-walker reset zeroes only the flagged walkers (after the copy)
        got = ctx.density_read(reset=[1, 0, 1])
        assert_counts(got, expected(S, [0, 1, 2, 0, 1, 2], Nbin, h, W))
        assert_counts(ctx.density_read(), expected(S, [1, 1], Nbin, h, W))
        # re-init resizes and zeroes
        ctx.density_init(5, 0.5 * h)
        got = ctx.density_read()
        assert got["planar"].shape == (W, 5, 5) and got["radial"].shape == (W, 5)
        assert all(not got[k].any() for k in got)
        ctx.density_accumulate([1])
        assert_counts(ctx.density_read(), expected(S, [1], 5, 0.5 * h, W))
        # bad arguments
        for Nbin_bad, h_bad in ((0, 1.0), (-3, 1.0), (4, 0.0), (4, -1.0), (4, float("nan"))):
            with pytest.raises(gpu_lib.PigsError):
                ctx.density_init(Nbin_bad, h_bad)
        ctx.density_init(4, 1.0)
        for bad in ([3], [-1], [0, 5]):
            with pytest.raises(gpu_lib.PigsError):
                ctx.density_accumulate(bad)
        with pytest.raises(gpu_lib.PigsError):
            ctx.density_accumulate(list(range(W)) + [W])
    # a periodic context
    pcfg = SystemConfig(dim=3, Np=16, Nb=2)
    VT, WF = gpu_lib.build_tables(pcfg)
    with gpu_lib.PigsContext(pcfg, VT, WF, n_walkers=1) as ctx:
        with pytest.raises(gpu_lib.PigsError, match="trapped"):
            ctx.density_init(10, 1.0)


# ---- driven by the device-resident sampler (K6, trap form) ------------------------------------------------------------
TRAP3D = """&system
 dim = 3, Np = 8, density = 0.365d0, trap = T
/
&samp
 resume = F, dt = 1.0d-2, Nb = 8, seed = 21, delta_cm = 0.12d0, CMFreq = 1,
 sampling = 'bis', Lstag = 4, Nlev = 2, Nstag = 2,
 Nblock = 2, Nstep = 10, Nbin = 60, Nk = 50
/
&obdm
 swapping = T, CWorm = 0.0d0, Nobdm = 0, Npw = 0
/
&wavefun
 Nmax = 10000, wf_table = T, v_table = T
/
&jastrow
 Rm = 1.20d0
/
&extpot
 a_ho = 1.0d0 1.3d0 0.8d0
/
"""


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


@pytest.mark.parametrize("which", ["trap2d", "trap3d"])
def test_driven_by_the_device_sampler(gpu_lib, oracle, which):
    if which == "trap2d":
        cfg = SystemConfig.from_namelists(open(os.path.join(RUNS, "trap2d_bis_cworm0", "vpi.in")).read())
    else:
        cfg = SystemConfig.from_namelists(TRAP3D)
    W, nstep = 4, 30
    h = cfg.rcut / 2.0
    Nbin = cfg.Nbin
    ctx = _k6_context(gpu_lib, oracle, cfg, W)
    try:
        ctx.density_init(Nbin, h)
        want = expected(np.zeros((W, cfg.Np, cfg.dim)), [], Nbin, h, W)
        for istep in range(1, nstep + 1):
            ctx.sampler_step(istep)
            ctx.density_accumulate()
            R = ctx.slice_download(cfg.Nb)
            e = expected(R, range(W), Nbin, h, W)
            for k in want:
                want[k] += e[k]
        got = ctx.density_read()
        assert_counts(got, want)
        assert got["samples"].tolist() == [nstep] * W
        assert np.all(got["planar"].sum(axis=tuple(range(1, got["planar"].ndim))) == nstep * cfg.Np)   # all inside
        assert np.all(got["pair"].sum(axis=1) == nstep * cfg.Np * (cfg.Np - 1))
    finally:
        ctx.close()


def test_accumulate_sees_the_worldline_queued_before_it(gpu_lib, oracle):
    """Context A: step, accumulate, step (no synchronisation in between), read.  Context B, same seeds: step, slice Nb.
    A's counts are those of B's slice: the accumulate saw the first step's worldline, never the second's."""
    cfg = SystemConfig.from_namelists(open(os.path.join(RUNS, "trap2d_bis_cworm0", "vpi.in")).read())
    W, h, Nbin = 4, cfg.rcut / 2.0, cfg.Nbin
    A = _k6_context(gpu_lib, oracle, cfg, W)
    B = _k6_context(gpu_lib, oracle, cfg, W)
    try:
        A.density_init(Nbin, h)
        A.sampler_step(1)
        A.density_accumulate()
        A.sampler_step(2)
        got = A.density_read()
        B.sampler_step(1)
        R = B.slice_download(cfg.Nb)
        assert_counts(got, expected(R, range(W), Nbin, h, W))
        B.sampler_step(2)
        R2 = B.slice_download(cfg.Nb)
        assert not np.array_equal(R, R2)                  # the second step moved something: the check has teeth
    finally:
        A.close()
        B.close()


# ---- the front end ------------------------------------------------------------------------------------------------------
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


def _check_integrals(d, cfg, suffix=""):
    """dens_vpi integrates (sum of mean * b^min(dim,2)) to Np, rho_vpi to Np, pr_vpi to Np-1 (shells of the d-ball)."""
    from pathintegralgroundstate_amd.profiles import bin_widths, shell_volumes
    h, Nbin, dim = cfg.rcut / 2.0, cfg.Nbin, cfg.dim
    b, _ = bin_widths(Nbin, h)
    dv = shell_volumes(dim, Nbin, h)
    dens = np.loadtxt(os.path.join(d, f"dens_vpi{suffix}.out"))
    assert dens.shape == (Nbin ** min(dim, 2), 2 + min(dim, 2))
    assert np.sum(dens[:, -2]) * b ** min(dim, 2) == pytest.approx(cfg.Np, rel=1e-8)
    for f, want in (("rho_vpi", cfg.Np), ("pr_vpi", cfg.Np - 1)):
        a = np.loadtxt(os.path.join(d, f"{f}{suffix}.out"))
        assert a.shape == (Nbin, 3)
        assert np.sum(a[:, 1] * dv) == pytest.approx(want, rel=1e-8), f
    if dim >= 2:
        # gnuplot layout: x fastest, a blank line after each y row
        rows = open(os.path.join(d, f"dens_vpi{suffix}.out")).read().split("\n\n")
        assert len([r for r in rows if r.strip()]) == Nbin


@pytest.mark.parametrize("name", ["trap2d_bis_cworm0", "ho1d_n2"])
def test_front_end_writes_the_profiles_and_changes_nothing_else(exe, name, tmp_path):
    txt = open(os.path.join(RUNS, name, "vpi.in")).read()
    cfg = SystemConfig.from_namelists(txt)
    off, on = str(tmp_path / "off"), str(tmp_path / "on")
    _run(exe, txt, off)
    out = _run(exe, txt + f"&gpu\n {KEY}\n/\n", on)
    assert "Density profiles" in out
    old = _files(off)
    assert _files(on) == sorted(old + list(NEW_FILES))
    assert not set(NEW_FILES) & set(old)
    for f in old:
        assert _same(off, on, f), f
    _check_integrals(on, cfg)
    # the two samplers: the same files
    dev = {}
    for ds in ("T", "F"):
        d = str(tmp_path / f"ds_{ds}")
        _run(exe, txt + f"&gpu\n device_sampler = {ds}, {KEY}\n/\n", d)
        dev[ds] = d
    for f in NEW_FILES:
        assert _same(dev["T"], dev["F"], f), f
        assert _same(dev["T"], on, f), f


def test_front_end_sharded_contexts_one_gpu(exe, tmp_path):
    """n_walkers = 4 on two contexts of this GPU against one context: per-walker files byte-identical, walker-averaged
    files to summation order (the block profiles meet in the all-reduced block vector)."""
    txt = open(os.path.join(RUNS, "trap2d_bis_cworm0", "vpi.in")).read()
    cfg = SystemConfig.from_namelists(txt)
    a, b = str(tmp_path / "one"), str(tmp_path / "sharded")
    _run(exe, txt + f"&gpu\n n_walkers = 4, device = 0, n_gpus = 1, {KEY}\n/\n", a)
    _run(exe, txt + f"&gpu\n n_walkers = 4, device = 0, n_gpus = 2, same_device = T, {KEY}\n/\n", b)
    for w in range(4):
        for f in ("dens_vpi", "rho_vpi", "pr_vpi", "e_vpi"):
            assert _same(a, b, f"{f}.w{w:04d}.out"), (f, w)
        _check_integrals(a, cfg, f".w{w:04d}")
    for f in NEW_FILES:
        x, y = np.loadtxt(os.path.join(a, f)), np.loadtxt(os.path.join(b, f))
        ok = np.isfinite(x)
        assert x.shape == y.shape and np.array_equal(ok, np.isfinite(y))
        assert np.all(np.abs(x - y)[ok] <= 1e-9 * np.abs(x[ok]) + 1e-300), f
    _check_integrals(a, cfg)


def test_front_end_host_driven_fallback_writes_the_profiles(exe, tmp_path):
    """A trapped Nlev = 5 input: K6's trap form stops at four levels, the front end falls back to the host-driven
    sampler, and the profiles are still written."""
    txt = """&system
 dim = 2, Np = 6, density = 0.1d0, trap = T
/
&samp
 resume = F, dt = 1.0d-2, Nb = 20, seed = 11, delta_cm = 0.2d0, CMFreq = 1, sampling = 'bis', Lstag = 4, Nlev = 5, Nstag = 2,
 Nblock = 2, Nstep = 5, Nbin = 50, Nk = 10
/
&obdm
 swapping = T, CWorm = 0.0d0, Nobdm = 0, Npw = 0
/
&wavefun
 Nmax = 4000, wf_table = T, v_table = T
/
&jastrow
 Rm = 1.10d0
/
&extpot
 a_ho = 1.0d0 1.3d0
/
"""
    out = _run(exe, txt + f"&gpu\n {KEY}\n/\n", str(tmp_path))
    assert "host-driven (the device-resident sampler does not serve" in out
    _check_integrals(str(tmp_path), SystemConfig.from_namelists(txt))


def test_front_end_refuses_the_key_for_a_periodic_system(exe, tmp_path):
    txt = open(os.path.join(RUNS, "he4_worm_s1982", "vpi.in")).read()
    out = _run(exe, txt + f"&gpu\n {KEY}\n/\n", str(tmp_path), expect_rc=2)
    assert "density_profile" in out and "trapped" in out
    assert not any(os.path.exists(tmp_path / f) for f in NEW_FILES)
