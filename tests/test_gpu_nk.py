"""The momentum distribution n(k) and the one-body density matrix on the MI355X (pigs_nk_*, pigs_nk.hip), through the C ABI.

The expected sums come from the numpy restatement in tests/nk_numpy.py (a straight np.cos of k.x per sample and vector).
The integer counts H, nopen and ninside are compared exactly; the cosine sums within 1e-12 per unit-modulus term, i.e.
1e-12 * nopen per (walker, vector): the project's S(k) bound of test_gpu_sqv.py.  Every (walker, vector) is compared in
every case."""
import os
import re

import numpy as np
import pytest

from conftest import GOLDEN, ROOT
from helpers import same_bits
from nk_numpy import half_space, sums
from pathintegralgroundstate_amd import SystemConfig

pytestmark = pytest.mark.gpu
RUNS = os.path.join(GOLDEN, "vpi_runs")
BOX = {2: [3.0, 4.5], 3: [3.0, 4.5, 3.75]}


def _status_codes():
    txt = open(os.path.join(ROOT, "include", "pigs_hip.h")).read()
    return {k: int(v) for k, v in re.findall(r"^\s*(PIGS_\w+)\s*=\s*(-?\d+)", txt, flags=re.M)}


def _tile():
    txt = open(os.path.join(ROOT, "include", "pigs_hip.h")).read()
    return int(re.search(r"#define\s+PIGS_NK_TILE\s+(\d+)", txt).group(1))


ST = _status_codes()
TILE = _tile()


def _cfg(dim, Np=4, Nb=2):
    L = BOX[dim]
    return SystemConfig(dim=dim, Np=Np, Nb=Nb, Lbox=L, density=Np / float(np.prod(L)))


def _context(gpu_lib, cfg, W):
    VT, WF = gpu_lib.build_tables(cfg)
    return gpu_lib.PigsContext(cfg, VT, WF, n_walkers=W)


def _pairs(rng, cfg, ns):
    """ns head/tail pairs anywhere in the box, the first ones on the edges of the fold: a difference of exactly +L_k/2 and
    -L_k/2, one ulp beyond either, and head = tail."""
    dim = cfg.dim
    L = np.asarray(cfg.Lbox[:dim])
    x = rng.uniform(-0.5, 0.5, (ns, 2, dim)) * L
    edge = []
    for k in range(dim):
        for head in (0.5 * L[k], -0.5 * L[k], np.nextafter(0.5 * L[k], np.inf), np.nextafter(-0.5 * L[k], -np.inf)):
            p = rng.uniform(-0.25, 0.25, (2, dim)) * L
            p[0, k], p[1, k] = head, 0.0                     # head - 0 is exact
            edge.append(p)
        p = rng.uniform(-0.25, 0.25, (2, dim)) * L
        p[0, k], p[1, k] = 0.25 * L[k], -0.25 * L[k]         # L/4 - (-L/4) = L/2 exactly
        edge.append(p)
    same = rng.uniform(-0.5, 0.5, dim) * L
    edge.append(np.stack([same, same]))
    edge = np.stack(edge)
    m = min(ns, len(edge))
    x[:m] = edge[:m]
    return x


def _want(cfg, W, listing, nmax, nbin):
    """listing: (walker, pairs) in list order -> the dict of nk_read that the listing adds to zeroed sums."""
    dim = cfg.dim
    nq = ((2 * nmax + 1) ** dim - 1) // 2
    out = {"C": np.zeros((W, nq)), "H": np.zeros((W,) + (nbin,) * dim, np.int64), "nopen": np.zeros(W, np.int64),
           "ninside": np.zeros(W, np.int64)}
    for w, x in listing:
        s = sums(x, cfg.Lbox, nmax, nbin, cfg.rcut2)
        for key in out:
            out[key][w] += s[key]
    return out


def _compare(got, want, what):
    for key in ("H", "nopen", "ninside"):
        assert got[key].dtype == np.int64 and np.array_equal(got[key], want[key]), (what, key)
    bound = 1e-12 * want["nopen"][:, None].astype(np.float64)
    err = np.abs(got["C"] - want["C"])
    ratio = np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0))
    worst = float(ratio.max())
    print(f"{what}: max |C - want| / (1e-12 nopen) = {worst:.3e} over {err.size} elements")
    assert np.all(np.isfinite(got["C"])) and np.all(err <= bound), (what, worst)
    return worst


# ---- 1. pigs_nk_add against the numpy restatement -------------------------------------------------------------------
@pytest.mark.parametrize("nbin", [1, 4])
@pytest.mark.parametrize("nmax", [1, 3])
@pytest.mark.parametrize("dim", [2, 3])
def test_add_matches_numpy(gpu_lib, dim, nmax, nbin):
    cfg = _cfg(dim)
    W = 6
    rng = np.random.default_rng(1000 * dim + 10 * nmax + nbin)
    counts = [0, 1, TILE, TILE + 1, 2 * TILE + 3, TILE]
    walkers = [0, 1, 2, 3, 4, 2]                             # walker 2 listed twice, walker 5 not at all
    listing = [(w, _pairs(rng, cfg, ns)) for w, ns in zip(walkers, counts)]
    with _context(gpu_lib, cfg, W) as ctx:
        ctx.nk_init(nmax, nbin)
        n = ctx.nk_vectors()
        assert n.dtype == np.int32 and np.array_equal(n, half_space(dim, nmax))
        ctx.nk_add(walkers, counts, np.concatenate([x for _, x in listing]))
        got = ctx.nk_read()
        want = _want(cfg, W, listing, nmax, nbin)
        assert want["nopen"].tolist() == [0, 1, 2 * TILE, TILE + 1, 2 * TILE + 3, 0]
        # samples sit on both sides of rcut and outside the grid's half-open cell (x_k = +L_k/2 exactly)
        assert 0 < want["ninside"].sum() < want["nopen"].sum() and want["H"].sum() < want["nopen"].sum()
        _compare(got, want, f"dim {dim} nmax {nmax} nbin {nbin}")
        # a second read has the same bits; reset zeroes the flagged walkers only
        again = ctx.nk_read(reset=np.array([0, 0, 1, 0, 0, 0], np.int32))
        assert all(same_bits(again[k], got[k]) for k in got)
        after = ctx.nk_read()
        for k in got:
            assert not after[k][2].any() and same_bits(np.delete(after[k], 2, 0), np.delete(got[k], 2, 0))


@pytest.mark.parametrize("dim,nmax", [(2, 64), (3, 16)])
def test_largest_grids_match_numpy(gpu_lib, dim, nmax):
    """The largest nmax that pigs_nk_init serves: the phasor tables pass 64 KiB of LDS in 2D, and a thread owns many
    vectors, over more than one tile."""
    cfg = _cfg(dim)
    rng = np.random.default_rng(5 + dim)
    x = _pairs(rng, cfg, TILE + 2)
    with _context(gpu_lib, cfg, 2) as ctx:
        ctx.nk_init(nmax, 3)
        ctx.nk_add([1], [len(x)], x)
        got = ctx.nk_read()
    _compare(got, _want(cfg, 2, [(1, x)], nmax, 3), f"dim {dim} nmax {nmax}")


@pytest.mark.parametrize("dim", [2, 3])
def test_lattice_of_samples_has_no_weight_off_zero(gpu_lib, dim):
    """The M^dim points x = j L/M: every k != 0 below M sums to zero, k = 0 to M^dim."""
    M, nmax = 4, 3
    cfg = _cfg(dim)
    L = np.asarray(cfg.Lbox[:dim])
    j = np.stack(np.meshgrid(*([np.arange(M)] * dim), indexing="ij"), -1).reshape(-1, dim)
    x = np.zeros((M ** dim, 2, dim))
    x[:, 0] = j * L / M
    with _context(gpu_lib, cfg, 1) as ctx:
        ctx.nk_init(nmax, M)
        ctx.nk_add([0], [M ** dim], x)
        got = ctx.nk_read()
    assert got["nopen"][0] == M ** dim
    worst = np.abs(got["C"]).max() / (1e-12 * M ** dim)
    print(f"dim {dim}: max |C(k != 0)| / (1e-12 M^dim) = {worst:.3e}")
    assert worst <= 1.0
    _compare(got, _want(cfg, 1, [(0, x)], nmax, M), f"lattice dim {dim}")


@pytest.mark.parametrize("dim", [2, 3])
def test_walker_listed_twice_counts_exactly_twice(gpu_lib, dim):
    cfg = _cfg(dim)
    rng = np.random.default_rng(77 + dim)
    x = _pairs(rng, cfg, TILE + 5)
    with _context(gpu_lib, cfg, 2) as ctx:
        ctx.nk_init(3, 4)
        ctx.nk_add([1], [len(x)], x)
        one = ctx.nk_read(reset=True)
        ctx.nk_add([1, 1], [len(x), len(x)], np.concatenate([x, x]))
        two = ctx.nk_read()
    assert one["nopen"][1] == len(x) and not one["C"][0].any()
    for k in one:
        assert same_bits(two[k], 2 * one[k]), k


# ---- 2. the sampler's end tape --------------------------------------------------------------------------------------
def _run_cfg(name="he4_worm_s1982"):
    return SystemConfig.from_namelists(open(os.path.join(RUNS, name, "vpi.in")).read())


def _worm_context(gpu_lib, oracle, cfg, seeds, Nobdm, Npw=0):
    """The worm fixture of test_gpu_sampler.py::test_device_sampler_worm_sector_vs_reference_program."""
    from oracle.pyoracle import System
    S = System(dim=cfg.dim, Np=cfg.Np, Nb=cfg.Nb, density=cfg.density, dt=cfg.dt)
    VT, WF = gpu_lib.build_tables(cfg)
    W = len(seeds)
    ctx = gpu_lib.PigsContext(cfg, VT, WF, n_walkers=W)
    ctx.sampler_init(CWorm=cfg.CWorm, swapping=cfg.swapping, Nobdm=Nobdm, Nbin=cfg.Nbin, Npw=Npw)
    Paths, xends = [], []
    for w, seed in enumerate(seeds):
        P, g = oracle.init_path(S, seed)
        Paths.append(P)
        xends.append(np.stack([P[cfg.Nb, cfg.Np - 1], P[cfg.Nb, cfg.Np - 1]]))
        ctx.sampler_set_rng(w, g.mti, np.array(g.mt[:], np.uint32))
    ctx.upload_all(np.stack(Paths))
    ctx.sampler_set_worm(np.zeros(W, np.int32), np.zeros(W, np.int32), np.stack(xends))
    return ctx


SEEDS = [1982, 1983, 1984]
NSTEP = 60


def test_tape_of_one_sample_is_the_step_s_end_to_end_vector(gpu_lib, oracle):
    """Nobdm = 1: the one sample of a step that ends open is the xend that pigs_sampler_get_worm returns after it."""
    cfg = _run_cfg()
    W, nmax, nbin = len(SEEDS), 3, 4
    ctx = _worm_context(gpu_lib, oracle, cfg, SEEDS, Nobdm=1)
    try:
        ctx.nk_init(nmax, nbin)
        ctx.nk_accumulate()                                  # before the first step: nothing
        assert not any(v.any() for v in ctx.nk_read().values())
        listing, open_steps = [], 0
        for istep in range(1, NSTEP + 1):
            ctx.sampler_step(istep)
            ctx.nk_accumulate()
            isopen, _, xend = ctx.sampler_get_worm()
            listing += [(w, xend[w][None]) for w in range(W) if isopen[w]]
            open_steps += int(isopen.sum())
            got = ctx.nk_read()
            _compare(got, _want(cfg, W, listing, nmax, nbin), f"step {istep}")
            assert got["nopen"].sum() == open_steps
        assert 0 < open_steps < W * NSTEP                    # steps ended open and steps ended closed
        # a second call after the same step counts that step again
        before = ctx.nk_read()
        ctx.nk_accumulate()
        after = ctx.nk_read()
        assert np.array_equal(after["nopen"] - before["nopen"], isopen.astype(np.int64))
    finally:
        ctx.close()


@pytest.mark.parametrize("split", [0, 1])
def test_tape_of_three_samples_against_the_obdm_histogram(gpu_lib, oracle, split):
    """split = 1: the stage-machine form of the step, in which the worm loop runs in a launch of its own (parts = 4) after
    the open / close attempt and the diagonal moves ran in two others."""
    cfg = _run_cfg()
    W = len(SEEDS)
    ctx = _worm_context(gpu_lib, oracle, cfg, SEEDS, Nobdm=3)
    try:
        ctx.set_tuning("sweep_split", split)
        ctx.nk_init(2, 5)
        ended_open = np.zeros(W, np.int64)
        for istep in range(1, NSTEP + 1):
            ctx.sampler_step(istep)
            ctx.nk_accumulate(list(range(W)))
            ended_open += ctx.sampler_events()[:, 1]
        got = ctx.nk_read()
        nrho = ctx.sampler_nrho()
        assert bool(ctx.sampler_form()["stage_machine"]) == bool(split)
    finally:
        ctx.close()
    assert ended_open.sum() > 0
    assert np.array_equal(got["nopen"], 3 * ended_open)
    assert np.array_equal(got["ninside"], nrho[:, :, 0].sum(axis=1).astype(np.int64))
    assert np.array_equal(nrho[:, :, 0], np.round(nrho[:, :, 0]))
    assert np.array_equal(got["H"].reshape(W, -1).sum(axis=1), got["nopen"])
    assert 0 < got["ninside"].sum() <= got["nopen"].sum()


def test_sampler_is_unchanged_by_the_tap(gpu_lib, oracle):
    """Same seeds with and without nk_init / nk_accumulate interleaved: the same bits everywhere."""
    cfg = _run_cfg()
    W = len(SEEDS)
    res = []
    for with_nk in (False, True):
        ctx = _worm_context(gpu_lib, oracle, cfg, SEEDS, Nobdm=cfg.Nobdm, Npw=cfg.Npw)
        try:
            if with_nk:
                ctx.nk_init(3, 4)
            events = []
            for istep in range(1, 31):
                ctx.sampler_step(istep)
                if with_nk:
                    ctx.nk_accumulate()
                events.append(ctx.sampler_events().copy())
            res.append((ctx.download_all(), ctx.sampler_nrho(), np.stack(events), ctx.sampler_counters16(),
                        [ctx.sampler_get_rng(w) for w in range(W)], ctx.sampler_get_worm()))
            if with_nk:
                assert ctx.nk_read()["nopen"].sum() > 0
        finally:
            ctx.close()
    a, b = res
    assert same_bits(a[0], b[0]) and same_bits(a[1], b[1])
    assert np.array_equal(a[2], b[2]) and np.array_equal(a[3], b[3])
    for (ma, sa), (mb, sb) in zip(a[4], b[4]):
        assert ma == mb and np.array_equal(sa, sb)
    assert np.array_equal(a[5][0], b[5][0]) and np.array_equal(a[5][1], b[5][1]) and same_bits(a[5][2], b[5][2])


# ---- 3. refusals ---------------------------------------------------------------------------------------------------
def _status(gpu_lib, call):
    with pytest.raises(gpu_lib.PigsError) as e:
        call()
    m = re.search(r"status (-?\d+)", str(e.value))
    assert m, str(e.value)
    return int(m.group(1))


def test_refusals(gpu_lib):
    ARG, UNS = ST["PIGS_ERR_ARG"], ST["PIGS_ERR_UNSUPPORTED"]
    trap = SystemConfig(dim=2, Np=6, Nb=2, trap=True, a_ho=[1.0, 1.3], Nmax=2000, Rm=1.2, dt=0.01)
    with _context(gpu_lib, trap, 1) as ctx:
        assert _status(gpu_lib, lambda: ctx.nk_init(2, 4)) == UNS
    for dim, big_n, big_b in ((2, 65, 1025), (3, 17, 129)):
        cfg = _cfg(dim)
        with _context(gpu_lib, cfg, 2) as ctx:
            assert _status(gpu_lib, lambda: ctx.nk_accumulate()) == ARG          # before nk_init
            assert _status(gpu_lib, lambda: ctx.nk_add([0], [0], np.zeros((0, 2, dim)))) == ARG
            for nmax, nbin in ((0, 4), (-1, 4), (big_n, 4), (2, 0), (2, -3), (2, big_b)):
                assert _status(gpu_lib, lambda: ctx.nk_init(nmax, nbin)) == ARG, (nmax, nbin)
            ctx.nk_init(big_n - 1, 4)                                            # the limits themselves are served
            ctx.nk_init(2, 4)
            assert _status(gpu_lib, lambda: ctx.nk_accumulate()) == ARG          # no sampler
            ctx.sampler_init()                                                   # CWorm = 0
            assert _status(gpu_lib, lambda: ctx.nk_accumulate()) == ARG
            x = np.zeros((1, 2, dim))
            assert _status(gpu_lib, lambda: ctx.nk_add([2], [1], x)) == ARG      # walker out of range
            assert _status(gpu_lib, lambda: ctx.nk_add([-1], [1], x)) == ARG
            one, neg = np.array([0], np.int32), np.array([-1], np.int32)
            ip, dp = ctx.L.pigs_nk_add.argtypes[2], ctx.L.pigs_nk_add.argtypes[4]
            assert ctx.L.pigs_nk_add(ctx.h, 1, one.ctypes.data_as(ip), neg.ctypes.data_as(ip), x.ctypes.data_as(dp)) == ARG
            rc = ctx.L.pigs_nk_add(ctx.h, -1, None, None, None)
            assert rc == ARG
            rc = ctx.L.pigs_nk_accumulate(ctx.h, -1, None)
            assert rc == ARG
            assert not any(v.any() for v in ctx.nk_read().values())              # a refused call adds nothing


# ---- 4. the front end ------------------------------------------------------------------------------------------------
PRINT = 1.0000001e-9            # the files carry 10 significant digits
FILES = ("nkvec_vpi", "nk_vpi", "n0_vpi", "nrvec_vpi")


@pytest.fixture(scope="module")
def exe(gpu_lib):
    import subprocess
    host = os.path.join(ROOT, "pathintegralgroundstate_amd", "host")
    subprocess.check_call(["make", "-s", "-C", host])
    return os.path.join(host, "pigs_vpi")


def _close(got, want, what):
    tol = PRINT * np.abs(want) + 1e-13 * np.abs(want).max()
    assert got.shape == want.shape and np.all(np.abs(got - want) <= tol), (what, np.abs(got - want).max())


def _close_err(got, x, what):
    """the error column: the root of a difference of two moments of the block values x [blocks, ..]"""
    nb = x.shape[0]
    m = x.mean(axis=0)
    err = np.sqrt(np.maximum((x * x).mean(axis=0) - m * m, 0.0) / nb)
    slack = np.sqrt(4.0 * np.abs(m) * PRINT * np.abs(m) / nb) + PRINT * err + 1e-13 * np.abs(m).max()
    assert np.all(np.abs(got - err) <= slack), (what, np.abs(got - err).max())


@pytest.mark.parametrize("device_sampler", ["T", "F"])
def test_front_end_writes_the_four_files(gpu_lib, oracle, exe, tmp_path, device_sampler):
    """he4_worm_s1982 with two walkers, momentum = T, with the device sampler (pigs_nk_accumulate after each step) and the
    host-driven one (pigs_nk_add where the OBDM histogram is taken): the old files byte for byte, and the four new files
    against profiles.normalize_nk / normalize_nrvec of the API's sums for the same seeds, normalised in the blocks in which
    nr_vpi.out is, with its zconf."""
    from pathintegralgroundstate_amd.profiles import normalize_nk, normalize_nrvec
    from test_gpu_front_end_blocks import _input, _run as run_vpi
    W, Nblock, Nstep, nmax, nbin = 2, 6, 25, 2, 4
    txt, cfg = _input("he4_worm_s1982", Nblock, Nstep)
    plain, on = str(tmp_path / "plain"), str(tmp_path / "on")
    base = f"&gpu\n n_walkers = {W}, device_sampler = {device_sampler}"
    run_vpi(exe, txt + base + "\n/\n", plain)
    out = run_vpi(exe, txt + base + f", momentum = T, nk_nmax = {nmax}, nk_nbin = {nbin}\n/\n", on)
    assert "Momentum n(k), n0" in out
    old = sorted(os.listdir(plain))
    new = sorted(set(os.listdir(on)) - set(old))
    assert sorted(f for f in new if ".w" not in f) == sorted(f + ".out" for f in FILES) and len(new) == 4 * (W + 1), new
    for f in old:
        if f not in ("stdout.txt", "vpi.in"):
            assert open(os.path.join(plain, f), "rb").read() == open(os.path.join(on, f), "rb").read(), f
    # the same chains through the API
    ctx = _worm_context(gpu_lib, oracle, cfg, [cfg.seed + w for w in range(W)], Nobdm=cfg.Nobdm, Npw=cfg.Npw)
    per = [[] for _ in range(W)]                              # (block, normalize_nk, rho1) of the blocks a walker normalises
    try:
        ctx.nk_init(nmax, nbin)
        n = ctx.nk_vectors()
        aux = np.zeros(W, np.int64)
        for b in range(1, Nblock + 1):
            for istep in range(1, Nstep + 1):
                ctx.sampler_step(istep)
                ctx.nk_accumulate()
                aux += ctx.sampler_events()[:, 1] == 0
            norm = aux // Nstep >= 1
            raw = ctx.nk_read(reset=norm.astype(np.int32))
            for w in np.flatnonzero(norm):
                one = {k: v[w] for k, v in raw.items()}
                per[w].append((b, normalize_nk(one, cfg.CWorm, float(aux[w]), cfg.Nobdm, cfg.Np, n=n, Lbox=cfg.Lbox),
                               normalize_nrvec(one, cfg.CWorm, float(aux[w]), cfg.Nobdm, cfg.density, cfg.Lbox, cfg.dim)["rho1"]))
                aux[w] = 0
        final = ctx.download_all()
    finally:
        ctx.close()
    assert np.array_equal(np.fromfile(os.path.join(on, "worldlines_final.bin")).reshape(final.shape), final)
    assert all(len(p) >= 2 for p in per) and sum(p[1]["nk0"] for q in per for p in q) > 0
    dim = cfg.dim

    def check(suffix, blocks):
        """blocks: (block number, vector values with n = 0 first, shell values, rho1) per counted block"""
        num = np.array([b[0] for b in blocks], float)
        vec, sh, rho = (np.stack([b[i] for b in blocks]) for i in (1, 2, 3))
        t = np.loadtxt(os.path.join(on, f"nkvec_vpi{suffix}.out"), ndmin=2)
        assert t.shape == (len(n) + 1, dim + 3) and not t[0, :dim + 1].any() and np.array_equal(t[1:, :dim], n)
        _close(t[:, dim + 1], vec.mean(axis=0), "nkvec" + suffix)
        _close_err(t[:, dim + 2], vec, "nkvec" + suffix)
        t0 = np.loadtxt(os.path.join(on, f"n0_vpi{suffix}.out"), ndmin=2)
        assert t0.shape == (len(blocks), 3) and np.array_equal(t0[:, 0], num)
        _close(t0[:, 2], vec[:, 0], "n0" + suffix)
        _close(t0[:, 1], vec[:, 0] / cfg.Np, "n0" + suffix)
        assert abs(t[0, dim + 1] - t0[:, 1].mean() * cfg.Np) <= 2 * PRINT * t[0, dim + 1]     # the n = 0 line is n0 Np
        ts = np.loadtxt(os.path.join(on, f"nk_vpi{suffix}.out"), ndmin=2)
        _close(ts[:, 1], sh.mean(axis=0), "nk" + suffix)
        _close(ts[:, 0], blocks[0][4], "nk" + suffix)
        tr = np.loadtxt(os.path.join(on, f"nrvec_vpi{suffix}.out"), ndmin=2)
        assert tr.shape == (nbin ** dim, dim + 2)
        _close(tr[:, dim], rho.mean(axis=0), "nrvec" + suffix)
        _close_err(tr[:, dim + 1], rho, "nrvec" + suffix)

    for w in range(W):
        check(f".w{w:04d}", [(b, np.r_[p["nk0"], p["nk"]], p["nk_shell"], r.ravel(), p["k"]) for b, p, r in per[w]])
    # the walker averages: over the walkers that normalised the block; the shells are those of the averaged vectors
    from pathintegralgroundstate_amd.profiles import shell_average
    av = []
    for b in range(1, Nblock + 1):
        got = [(p, r) for q in per for bb, p, r in q if bb == b]
        if got:
            v = np.mean([np.r_[p["nk0"], p["nk"]] for p, _ in got], axis=0)
            k, shm, _ = shell_average(n, cfg.Lbox, v[1:])
            av.append((b, v, shm, np.mean([r.ravel() for _, r in got], axis=0), k))
    check("", av)


def test_front_end_sharded_contexts_one_gpu(exe, tmp_path):
    """n_walkers = 4 on two contexts of this GPU against one context: per-walker files byte-identical, the walker-averaged
    files equal up to summation order (the block values meet in the all-reduced block vector)."""
    from test_gpu_front_end_blocks import _run as run_vpi
    txt = open(os.path.join(RUNS, "he4_worm_s1982", "vpi.in")).read()
    key = "momentum = T, nk_nmax = 2, nk_nbin = 4, sq_vector = T, sq_nmax = 2"
    a, b = str(tmp_path / "one"), str(tmp_path / "sharded")
    run_vpi(exe, txt + f"&gpu\n n_walkers = 4, device = 0, n_gpus = 1, {key}\n/\n", a)
    run_vpi(exe, txt + f"&gpu\n n_walkers = 4, device = 0, n_gpus = 2, same_device = T, {key}\n/\n", b)
    for w in range(4):
        for f in FILES + ("nr_vpi", "sqvec_vpi", "e_vpi"):
            name = f"{f}.w{w:04d}.out"
            assert open(os.path.join(a, name), "rb").read() == open(os.path.join(b, name), "rb").read(), name
    # (file, column of the means, column of the errors)
    for f, mean, err in (("nkvec_vpi.out", [4], [5]), ("nk_vpi.out", [1], [2]), ("n0_vpi.out", [1, 2], []),
                         ("nrvec_vpi.out", [3], [4])):
        x, y = np.loadtxt(os.path.join(a, f), ndmin=2), np.loadtxt(os.path.join(b, f), ndmin=2)
        assert x.shape == y.shape and x.shape[0] > 0 and np.all(np.isfinite(x)) and np.all(np.isfinite(y)), f
        d = np.abs(x - y)
        other = [c for c in range(x.shape[1]) if c not in mean + err]
        assert np.all(d[:, other] == 0), f
        mtol = PRINT * np.abs(x[:, mean]) + 1e-13 * np.abs(x[:, mean]).max()
        assert np.all(d[:, mean] <= mtol), f
        if err:
            assert np.all(d[:, err] <= np.sqrt(4.0 * np.abs(x[:, mean]) * mtol) + PRINT * np.abs(x[:, err])), f


def test_front_end_refuses_the_key_without_a_worm_sector_or_in_a_trap(exe, tmp_path):
    import subprocess
    for i, (name, word) in enumerate((("he4_bis_cworm0_s1982", "CWorm"), ("trap2d_bis_cworm0", "periodic"))):
        wd = tmp_path / str(i)
        os.makedirs(wd)
        txt = open(os.path.join(RUNS, name, "vpi.in")).read() + "&gpu\n momentum = T\n/\n"
        r = subprocess.run([exe], input=txt.encode(), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, cwd=wd, timeout=120)
        out = r.stdout.decode(errors="replace")
        assert r.returncode == 2 and "momentum" in out and word in out, out[-2000:]
        assert not os.path.exists(wd / "e_vpi.out")
