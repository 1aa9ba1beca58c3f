"""Imaginary-time profiles V(tau), virial and link lengths on the MI355X (pigs_tau_*, pigs_tau.hip), through the C ABI and
the front end.

The expected sums come from the numpy restatement in tests/tau_numpy.py (the reference's plain arithmetic, pinned to the
CPU oracle by tests/test_tau_host.py).  The bound per element is 1e-12 * sum|terms| from the numpy side: SURVEY section 7's
kernel tolerance in the form tests/test_gpu_fqt.py uses; W has terms of both signs, so a bound relative to the result would
be wrong.  No comparison masks or skips elements: every (walker, slice, quantity) is compared in every case.  The inputs
are jittered lattices (tau_numpy.lattice_paths / trap_paths): no pair comes near the NaN/-Inf head of the table (quirk Q4),
which every case asserts."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, ROOT
from helpers import same_bits
from pathintegralgroundstate_amd import SystemConfig
from pathintegralgroundstate_amd.profiles import pressure_virial
from tau_numpy import expected, lattice_paths, min_max_distance, tau_sums, trap_paths

pytestmark = pytest.mark.gpu
RUNS = os.path.join(GOLDEN, "vpi_runs")
HOST = os.path.join(ROOT, "pathintegralgroundstate_amd", "host")
DENSITY = {1: 0.2, 2: 0.25, 3: 0.365}
REL = 1e-10


def _status_codes():
    """The pigs_status values as include/pigs_hip.h declares them."""
    txt = open(os.path.join(ROOT, "include", "pigs_hip.h")).read()
    return {k: int(v) for k, v in re.findall(r"^\s*(PIGS_\w+)\s*=\s*(-?\d+)", txt, flags=re.M)}


ST = _status_codes()
assert ST["PIGS_OK"] == 0 and len({ST["PIGS_ERR_ARG"], ST["PIGS_ERR_HIP"], ST["PIGS_ERR_UNSUPPORTED"]}) == 3


def _cfg(dim, Np, Nb, trap=False):
    if trap:
        return SystemConfig(dim=dim, Np=Np, Nb=Nb, trap=True, a_ho=[1.0, 1.3, 0.8][:dim], Rm=1.2, dt=0.01)
    return SystemConfig(dim=dim, Np=Np, Nb=Nb, density=DENSITY[dim])


def _paths(cfg, W, rng):
    P = (trap_paths if cfg.trap else lattice_paths)(cfg, W, rng)
    lo, hi = min_max_distance(P, cfg)
    assert lo > 3 * cfg.dr and (not cfg.trap or hi < cfg.rcut - 2 * cfg.dr), (lo, hi)
    return P


def _assert_close(got, want, A, what=""):
    assert got.shape == want.shape, (got.shape, want.shape)
    assert np.all(np.isfinite(want)), what
    bound = 1e-12 * A
    err = np.abs(got - want)
    with np.errstate(all="ignore"):
        worst = float(np.max(np.where(err == 0, 0.0, err / bound)))
    print(f"{what}: max |got-want|/bound = {worst:.3e} over {got.size} elements")
    assert np.all(np.isfinite(got)) and np.all(err <= bound), (what, worst)


# ---- 1., 2. against the numpy restatement -----------------------------------------------------------------------------
@pytest.mark.parametrize("Nb", [1, 4])
@pytest.mark.parametrize("Np", [2, 3, 64, 256, 257, 300])
@pytest.mark.parametrize("dim", [1, 2, 3])
def test_periodic_matches_numpy(gpu_lib, dim, Np, Nb):
    """With Np = 2 an element is ONE term: the kernel's terms carry the reference's bits (the exact-term forms of
    pigs_device.h), so such an element matches whatever its size -- also where the pair sits next to the potential
    minimum (dim 2: a = L/2 = 1.41 against 1.16), v' passes through zero and the bound 1e-12 |r v'| vanishes with it."""
    W = 3
    cfg = _cfg(dim, Np, Nb)
    VT, WF = gpu_lib.build_tables(cfg)
    P = _paths(cfg, W, np.random.default_rng(100000 * dim + 100 * Np + Nb))
    with gpu_lib.PigsContext(cfg, VT, WF, n_walkers=W) as ctx:
        ctx.upload_all(P)
        ctx.tau_init()
        ctx.tau_accumulate()
        ctx.tau_accumulate()
        got = ctx.tau_read()
    Q, A, n = expected(P, list(range(W)) * 2, VT, cfg)
    assert got["Q"].shape == (W, 2 * Nb + 1, 4) and got["samples"].dtype == np.int64
    assert np.array_equal(got["samples"], n) and n.tolist() == [2] * W
    assert not got["Q"][:, :, 1].any() and not got["Q"][:, 2 * Nb, 3].any()          # exactly 0.0
    _assert_close(got["Q"], Q, A, f"periodic dim {dim} Np {Np} Nb {Nb}")


@pytest.mark.parametrize("Np", [2, 64, 257])
@pytest.mark.parametrize("dim", [1, 2, 3])
def test_trapped_matches_numpy(gpu_lib, dim, Np):
    W, Nb = 3, 4
    cfg = _cfg(dim, Np, Nb, trap=True)
    VT, WF = gpu_lib.build_tables(cfg)
    P = _paths(cfg, W, np.random.default_rng(7000 * dim + Np))
    with gpu_lib.PigsContext(cfg, VT, WF, n_walkers=W) as ctx:
        ctx.upload_all(P)
        ctx.tau_init()
        ctx.tau_accumulate()
        got = ctx.tau_read()
    Q, A, n = expected(P, range(W), VT, cfg)
    assert got["samples"].tolist() == [1] * W and np.all(Q[:, :, 1] > 0) and not got["Q"][:, 2 * Nb, 3].any()
    _assert_close(got["Q"], Q, A, f"trap dim {dim} Np {Np}")


# ---- 3. the cutoff decisions ------------------------------------------------------------------------------------------
def test_pairs_and_links_at_the_cutoff(gpu_lib):
    """2D, L = 4, rcut = 2: a pair just inside and a pair just outside rcut (along a diagonal: an axis pair beyond L/2
    folds back inside), and a link whose folded length exceeds rcut (quirk Q8's guard drops it from D2)."""
    cfg = _cfg(2, 4, 1)
    VT, WF = gpu_lib.build_tables(cfg)
    rc = cfg.rcut
    u = np.array([1.0, 1.0]) / np.sqrt(2.0)
    base = np.array([[-1.6, -1.7], [0, 0], [-1.5, 0.4], [0, 0]])
    base[1] = base[0] + rc * (1 - 1e-9) * u                   # pair (0,1) inside
    base[3] = base[2] + rc * (1 + 1e-9) * np.array([u[0], -u[1]])      # pair (2,3) outside
    P = np.stack([base, base, base])[None].copy()
    P[0, 1, 0] += [0.01, -0.02]
    P[0, 2, 2] = base[2] + [1.55, 1.5]                        # link of particle 2 between slices 1 and 2: |.| = 2.157 > rcut
    assert np.all(np.abs(P) < 0.5 * cfg.Lbox[0])
    lo, _ = min_max_distance(P, cfg)
    assert lo > 3 * cfg.dr
    Q, A, n = tau_sums(P[0], VT, cfg)
    assert n[0, 0] == 5 and n[0, 1] == 4 and n[1, 1] == 3, n  # 6 pairs, one outside; the long link is dropped
    d01 = base[0] - base[1]
    d23 = base[2] - base[3]
    assert 0 < cfg.rcut2 - d01 @ d01 < 1e-8 * cfg.rcut2 and 0 < d23 @ d23 - cfg.rcut2 < 1e-8 * cfg.rcut2
    with gpu_lib.PigsContext(cfg, VT, WF, n_walkers=1) as ctx:
        ctx.upload_all(P)
        ctx.tau_init()
        ctx.tau_accumulate()
        got = ctx.tau_read()["Q"]
    _assert_close(got[0], Q, A, "cutoff")
    # the decisions have teeth: the pair just inside carries far more than the bound, the dropped link too
    from tau_numpy import interpolate
    v_in = float(interpolate(0, cfg.Nmax, cfg.dr, VT, np.array([np.sqrt(d01 @ d01)]))[0])
    assert abs(v_in) > 1e3 * 1e-12 * A[0, 0] and 2.157 ** 2 > 1e3 * 1e-12 * A[1, 3]


# ---- 4. against existing kernels ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("Np", [64, 300])
def test_agrees_with_the_slice_hook_and_therm_energy(gpu_lib, Np):
    W, Nb = 2, 4
    cfg = _cfg(3, Np, Nb)
    VT, WF = gpu_lib.build_tables(cfg)
    P = _paths(cfg, W, np.random.default_rng(Np))
    with gpu_lib.PigsContext(cfg, VT, WF, n_walkers=W) as ctx:
        ctx.upload_all(P)
        ctx.tau_init()
        ctx.tau_accumulate()
        Q = ctx.tau_read()["Q"]
        for w in range(W):
            for b in range(2 * Nb + 1):
                want, _ = ctx.potential_energy_slice(w, b, False)
                assert abs(Q[w, b, 0] + Q[w, b, 1] - want) <= REL * abs(want), (w, b)
        _, _, Ep = ctx.therm_energy_batch()
        assert np.all(np.abs(Q[:, Nb, 0] + Q[:, Nb, 1] - Ep) <= REL * np.abs(Ep))


# ---- 5. semantics; 6. bits ----------------------------------------------------------------------------------------------
def _run_lists(gpu_lib, cfg, VT, WF, paths, lists):
    with gpu_lib.PigsContext(cfg, VT, WF, n_walkers=paths.shape[0]) as ctx:
        ctx.upload_all(paths)
        ctx.tau_init()
        for wl in lists:
            ctx.tau_accumulate(wl)
        return ctx.tau_read()


def test_semantics_of_lists_reset_and_reinit(gpu_lib):
    W, Nb = 5, 4
    cfg = _cfg(3, 64, Nb)
    VT, WF = gpu_lib.build_tables(cfg)
    P = _paths(cfg, W, np.random.default_rng(5))
    one = _run_lists(gpu_lib, cfg, VT, WF, P, [None])
    Q, A, _ = expected(P, range(W), VT, cfg)
    _assert_close(one["Q"], Q, A, "one call")
    twice = _run_lists(gpu_lib, cfg, VT, WF, P, [None, None])                 # x + x is exact
    assert same_bits(twice["Q"], 2.0 * one["Q"]) and twice["samples"].tolist() == [2] * W
    dup = _run_lists(gpu_lib, cfg, VT, WF, P, [[3, 3]])                       # listed twice: counts twice
    assert same_bits(dup["Q"][3], 2.0 * one["Q"][3]) and dup["samples"].tolist() == [0, 0, 0, 2, 0]
    assert not dup["Q"][[0, 1, 2, 4]].any()
    with gpu_lib.PigsContext(cfg, VT, WF, n_walkers=W) as ctx:
        ctx.upload_all(P)
        ctx.tau_init()
        ctx.tau_accumulate()
        ctx.tau_accumulate([4, 1])                                            # a sub-list leaves the others untouched
        got = ctx.tau_read(reset=[0, 1, 0, 0, 0])
        assert got["samples"].tolist() == [1, 2, 1, 1, 2]
        assert same_bits(got["Q"][[0, 2, 3]], one["Q"][[0, 2, 3]]) and same_bits(got["Q"][[1, 4]], 2.0 * one["Q"][[1, 4]])
        after = ctx.tau_read()                                                # the mask zeroed walker 1 only
        assert after["samples"].tolist() == [1, 0, 1, 1, 2] and not after["Q"][1].any()
        assert same_bits(after["Q"][[0, 2, 3, 4]], got["Q"][[0, 2, 3, 4]])
        ctx.tau_init()                                                        # a second init zeroes all
        z = ctx.tau_read()
        assert not z["Q"].any() and not z["samples"].any()
        ctx.tau_accumulate([2])
        assert same_bits(ctx.tau_read()["Q"][2], one["Q"][2])


def test_bits_do_not_depend_on_the_launch(gpu_lib):
    W, Nb = 5, 4
    cfg = _cfg(3, 64, Nb)
    VT, WF = gpu_lib.build_tables(cfg)
    P = _paths(cfg, W, np.random.default_rng(6))
    ref = _run_lists(gpu_lib, cfg, VT, WF, P, [None])["Q"]
    alone = _run_lists(gpu_lib, cfg, VT, WF, P[4:5], [None])["Q"]             # alone in a context of 1 walker
    assert same_bits(alone[0], ref[4])                                        # ... as walker 4 of 5
    perm = _run_lists(gpu_lib, cfg, VT, WF, P, [[3, 0, 4, 2, 1]])["Q"]
    assert same_bits(perm, ref)
    split = _run_lists(gpu_lib, cfg, VT, WF, P, [[4, 1], [0, 2, 3]])["Q"]
    assert same_bits(split, ref)
    # a list longer than 256 entries (repeats) against the same counts made in short calls
    long_list = [w % W for w in range(300)]
    a = _run_lists(gpu_lib, cfg, VT, WF, P, [long_list])
    b = _run_lists(gpu_lib, cfg, VT, WF, P, [None] * 60)
    assert a["samples"].tolist() == [60] * W and same_bits(a["Q"], b["Q"])


def test_more_than_256_walkers_in_one_list(gpu_lib):
    """300 distinct walkers behind one call (two launches) against the same worldlines six at a time."""
    W, Nb = 300, 2
    cfg = _cfg(2, 9, Nb)
    VT, WF = gpu_lib.build_tables(cfg)
    P6 = _paths(cfg, 6, np.random.default_rng(11))
    small = _run_lists(gpu_lib, cfg, VT, WF, P6, [None])["Q"]
    big = _run_lists(gpu_lib, cfg, VT, WF, P6[np.arange(W) % 6], [None, list(range(W - 1, -1, -1)) + [7, 7, 299]])
    cnt = np.full(W, 2)
    cnt[7] += 2
    cnt[299] += 1
    assert big["samples"].tolist() == cnt.tolist()
    want = np.stack([sum([small[w % 6]] * int(cnt[w] - 1), small[w % 6]) for w in range(W)])
    assert same_bits(big["Q"], want)


# ---- 7. a non-finite element stays local --------------------------------------------------------------------------------
def test_a_coincident_pair_stays_in_its_element(gpu_lib):
    W, Nb = 3, 4
    cfg = _cfg(3, 64, Nb)
    VT, WF = gpu_lib.build_tables(cfg)
    P = _paths(cfg, W, np.random.default_rng(8))
    Qc, Ac, _ = expected(P, range(W), VT, cfg)
    Pb = P.copy()
    Pb[1, 2, 17] = Pb[1, 2, 40]                               # one coincident pair in slice 2 of walker 1
    Qb, Ab, _ = expected(Pb, [1], VT, cfg)                    # (links 1 and 2 of particle 17 move too: finite)
    with gpu_lib.PigsContext(cfg, VT, WF, n_walkers=W) as ctx:
        ctx.upload_all(Pb)
        ctx.tau_init()
        ctx.tau_accumulate()
        got = ctx.tau_read(reset=[0, 1, 0])
        assert not np.isfinite(got["Q"][1, 2, 0]) and not np.isfinite(got["Q"][1, 2, 2])
        ok = np.ones((W, 2 * Nb + 1, 4), bool)
        ok[1, 2, 0] = ok[1, 2, 2] = False
        want, A = Qc.copy(), Ac.copy()
        want[1], A[1] = Qb[1], Ab[1]
        assert np.all(np.isfinite(want[ok]))
        _assert_close(got["Q"][ok], want[ok], A[ok], "all other elements")
        after = ctx.tau_read()                                # a reset clears it
        assert not after["Q"][1].any() and after["samples"].tolist() == [1, 0, 1]
        ctx.upload_all(P)
        ctx.tau_accumulate([1])
        _assert_close(ctx.tau_read()["Q"][1], Qc[1], Ac[1], "walker 1 afterwards")


# ---- 8. status codes ----------------------------------------------------------------------------------------------------
def test_status_codes(gpu_lib):
    W = 3
    cfg = _cfg(2, 9, 2)
    VT, WF = gpu_lib.build_tables(cfg)
    dp, lp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int64), C.POINTER(C.c_int32)
    Q = np.zeros((W, 5, 4))
    n = np.zeros(W, np.int64)
    with gpu_lib.PigsContext(cfg, VT, WF, n_walkers=W) as ctx:
        assert ctx.L.pigs_tau_accumulate(ctx.h, 1, None) == ST["PIGS_ERR_ARG"]          # before init
        assert ctx.L.pigs_tau_read(ctx.h, Q.ctypes.data_as(dp), n.ctypes.data_as(lp), None) == ST["PIGS_ERR_ARG"]
        with pytest.raises(gpu_lib.PigsError):
            ctx.tau_accumulate()
        assert ctx.L.pigs_tau_init(ctx.h) == ST["PIGS_OK"]
        assert ctx.L.pigs_tau_accumulate(ctx.h, -1, None) == ST["PIGS_ERR_ARG"]
        assert ctx.L.pigs_tau_accumulate(ctx.h, W + 1, None) == ST["PIGS_ERR_ARG"]      # 0..W: walker W out of range
        for bad in ([W], [-1], [0, W + 2]):
            wl = np.array(bad, np.int32)
            assert ctx.L.pigs_tau_accumulate(ctx.h, wl.size, wl.ctypes.data_as(ip)) == ST["PIGS_ERR_ARG"]
            with pytest.raises(gpu_lib.PigsError):
                ctx.tau_accumulate(bad)
        assert ctx.L.pigs_tau_read(ctx.h, None, n.ctypes.data_as(lp), None) == ST["PIGS_ERR_ARG"]
        assert ctx.L.pigs_tau_accumulate(ctx.h, 0, None) == ST["PIGS_OK"]
        got = ctx.tau_read()
        assert not got["Q"].any() and not got["samples"].any()                          # a refused list adds nothing


# ---- 9. a sampled state -------------------------------------------------------------------------------------------------
def test_matches_numpy_on_a_sampled_state(gpu_lib, oracle):
    from oracle.pyoracle import System
    cfg = SystemConfig.from_namelists(open(os.path.join(RUNS, "he4_bis_cworm0_s1982", "vpi.in")).read())
    W = 4
    S = System(dim=cfg.dim, Np=cfg.Np, Nb=cfg.Nb, density=cfg.density, dt=cfg.dt, trap=cfg.trap, a_ho=cfg.a_ho,
               Lbox=cfg.Lbox, rcut=cfg.rcut)
    VT, WF = gpu_lib.build_tables(cfg)
    ctx = gpu_lib.PigsContext(cfg, VT, WF, n_walkers=W)
    try:
        ctx.sampler_init()
        Paths = []
        for w in range(W):
            P, g = oracle.init_path(S, cfg.seed + w)
            Paths.append(P)
            ctx.sampler_set_rng(w, g.mti, np.array(g.mt[:], np.uint32))
        ctx.upload_all(np.stack(Paths))
        ctx.tau_init()
        Q = np.zeros((W, cfg.M, 4))
        A = np.zeros_like(Q)
        for istep in range(1, 4):
            ctx.sampler_step(istep)
            ctx.tau_accumulate()
            P = ctx.download_all()
            assert min_max_distance(P, cfg)[0] > 3 * cfg.dr
            e = expected(P, range(W), VT, cfg)
            Q, A = Q + e[0], A + e[1]
        got = ctx.tau_read()
        assert got["samples"].tolist() == [3] * W
        _assert_close(got["Q"], Q, A, "sampled state")
    finally:
        ctx.close()


# ---- 10. the front end --------------------------------------------------------------------------------------------------
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


def _short(txt):
    txt = re.sub(r"Nblock\s*=\s*\d+", "Nblock = 2", txt)
    return re.sub(r"Nstep\s*=\s*\d+", "Nstep = 3", txt)


def _rows(path):
    return [[float(t) for t in ln.split()] for ln in open(path) if ln.strip() and not ln.startswith("#")]


def test_front_end_periodic_run(exe, tmp_path):
    txt = _short(open(os.path.join(RUNS, "he4_cworm0", "vpi.in")).read())
    cfg = SystemConfig.from_namelists(txt)
    out = _run(exe, txt + "&gpu\n tau_profile = T, tau_window = 2\n/\n", str(tmp_path))
    assert "V(tau)" in out
    rows = _rows(tmp_path / "tau_vpi.out")
    M = 2 * cfg.Nb + 1
    assert len(rows) == M and [len(r) for r in rows] == [10] * (M - 1) + [8]
    assert [r[0] for r in rows] == list(range(M))
    assert np.allclose([r[1] for r in rows], [(b - cfg.Nb) * cfg.dt for b in range(M)], rtol=1e-9, atol=1e-300)
    assert all(r[4] == 0.0 and r[5] == 0.0 for r in rows)                               # Vext of a periodic system
    # row Nb against the potential energy per particle that the front end takes from ThermEnergy's Ep: column 4 of
    # et_vpi.out, one row per block.  Both files print 10 significant digits (each value within 5e-10 relative), the two
    # kernels agree far below that: the block mean of the one against the other's value to 1e-9 relative.
    et = np.loadtxt(tmp_path / "et_vpi.out").reshape(-1, 4)
    assert et.shape[0] == 2
    v = rows[cfg.Nb][2] + rows[cfg.Nb][4]
    assert abs(v - et[:, 3].mean()) <= 1.001e-9 * abs(v), (v, et[:, 3])
    head = open(tmp_path / "press_vpi.out").readline()
    assert head.startswith("#") and "rcut" in head
    pr = np.array(_rows(tmp_path / "press_vpi.out"))
    assert pr.shape == (2, 4) and pr[:, 0].tolist() == [1.0, 2.0]
    ev = np.loadtxt(tmp_path / "e_vpi.out").reshape(-1, 4)
    assert np.array_equal(pr[:, 2], ev[:, 2])                                           # Kin/N as e_vpi.out has it
    want = pressure_virial(pr[:, 2], pr[:, 1], cfg.density, cfg.dim)
    tol = 5.0000001e-10 * (np.abs(pr[:, 3]) + cfg.density / cfg.dim * (2 * np.abs(pr[:, 2]) + np.abs(pr[:, 1])))
    assert np.all(np.abs(pr[:, 3] - want) <= tol), (pr, want)


def test_front_end_walker_average(exe, tmp_path):
    """Three walkers: the unsuffixed files hold the walker average of the per-walker ones (every walker has a diagonal
    block in every block here, so the mean of the walkers' means is the mean of the block averages; 10 printed digits)."""
    txt = _short(open(os.path.join(RUNS, "he4_cworm0", "vpi.in")).read())
    cfg = SystemConfig.from_namelists(txt)
    _run(exe, txt + "&gpu\n n_walkers = 3, tau_profile = T, tau_window = 1\n/\n", str(tmp_path))
    M = 2 * cfg.Nb + 1
    av = _rows(tmp_path / "tau_vpi.out")
    per = [_rows(tmp_path / f"tau_vpi.w{w:04d}.out") for w in range(3)]
    assert [len(r) for r in av] == [10] * (M - 1) + [8]
    for b in range(M):
        for c in range(2, len(av[b]), 2):                                                # the mean columns
            x = np.array([p[b][c] for p in per])
            assert np.all(np.isfinite(x)) and abs(av[b][c] - x.mean()) <= 1.001e-9 * np.abs(x).max(), (b, c, av[b][c], x)
    pa = np.array(_rows(tmp_path / "press_vpi.out"))
    pw = np.array([_rows(tmp_path / f"press_vpi.w{w:04d}.out") for w in range(3)])
    assert pa.shape == (2, 4) and pw.shape == (3, 2, 4)
    assert np.all(np.abs(pa[:, 1:3] - pw[:, :, 1:3].mean(0)) <= 1.001e-9 * np.abs(pw[:, :, 1:3]).max(0))


def test_front_end_trapped_run(exe, tmp_path):
    txt = _short(open(os.path.join(RUNS, "trap2d_bis_cworm0", "vpi.in")).read())
    cfg = SystemConfig.from_namelists(txt)
    _run(exe, txt + "&gpu\n tau_profile = T\n/\n", str(tmp_path))
    rows = _rows(tmp_path / "tau_vpi.out")
    assert len(rows) == 2 * cfg.Nb + 1
    assert all(r[4] > 0.0 for r in rows) and np.all(np.isfinite([x for r in rows for x in r[:6]]))
    assert not os.path.exists(tmp_path / "press_vpi.out")
