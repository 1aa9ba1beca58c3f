"""The cluster-size distribution on the MI355X (pigs_cl_*, pigs_cl.hip), through the C ABI.

The expected sums come from the numpy restatement in tests/cl_numpy.py (a plain union-find over the bond list and the same
IEEE operations in the same order; pinned to a flood fill, to lattices and to the closed form of a chain by
tests/test_cl_numpy_host.py).  Every integer array must be EQUAL; rg2 lies within 1e-12 * Sum|terms| per element, the
project's bound for a fixed-order sum (the terms are non-negative, so Sum|terms| is the expected value itself), and has the
restatement's bits where an element holds one term.  No comparison masks or skips elements.

Largest |got - want| / bound seen on the MI355X: see DESIGN.md (the cluster section)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import cl_numpy as cn
from conftest import ROOT
from helpers import same_bits
from pathintegralgroundstate_amd import SystemConfig, api
from pathintegralgroundstate_amd.profiles import normalize_cl

pytestmark = pytest.mark.gpu
DENSITY = {1: 0.3, 2: 0.25, 3: 0.365}
INTS = ("nsize", "nlarge", "nbond", "samples")
_ip = C.POINTER(C.c_int32)


def _header():
    return open(os.path.join(ROOT, "include", "pigs_hip.h")).read()


ST = {k: int(v) for k, v in re.findall(r"^\s*(PIGS_\w+)\s*=\s*(-?\d+)", _header(), flags=re.M)}
assert ST["PIGS_OK"] == 0 and len({ST["PIGS_ERR_ARG"], ST["PIGS_ERR_HIP"], ST["PIGS_ERR_UNSUPPORTED"]}) == 3
ADJ_MAX = int(re.search(r"constexpr int kClAdjNpMax = (\d+);", open(os.path.join(
    ROOT, "pathintegralgroundstate_amd", "csrc", "pigs_kernels.h")).read()).group(1))


def _cfg(dim, Np, Nb, Lbox=None):
    """A box of unequal sides."""
    L = (Np / DENSITY[dim]) ** (1.0 / dim)
    Lbox = Lbox if Lbox is not None else [[L], [0.8 * L, 1.25 * L], [0.8 * L, 1.25 * L, L]][dim - 1]
    return SystemConfig(dim=dim, Np=Np, Nb=Nb, density=Np / float(np.prod(Lbox)), Lbox=Lbox)


def _assert_same(got, exp, what):
    for k in INTS:
        assert got[k].dtype == np.int64 and got[k].shape == exp[k].shape, (what, k)
        assert np.array_equal(got[k], exp[k]), (what, k, got[k], exp[k])
    assert got["rg2"].shape == exp["rg2"].shape and got["rg2"].dtype == np.float64, what
    bound = 1e-12 * np.abs(exp["rg2"])
    err = np.abs(got["rg2"] - exp["rg2"])
    with np.errstate(all="ignore"):
        worst = float(np.max(np.where(err == 0, 0.0, err / bound), initial=0.0))
    print(f"{what}: max |got-want|/bound of rg2 = {worst:.3e} over {err.size} elements")
    assert np.all(err <= bound), (what, worst)
    one = exp["terms"] <= 1
    assert same_bits(got["rg2"][one], exp["rg2"][one]), (what, "an element of one term")


def _run(gpu_lib, cfg, P, rc, window, lists, also=None):
    VT, WF = gpu_lib.build_tables(cfg)
    with gpu_lib.PigsContext(cfg, VT, WF, n_walkers=P.shape[0]) as ctx:
        ctx.upload_all(P)
        ctx.cl_init(rc, window)
        for wl in lists:
            ctx.cl_accumulate(wl)
        got = ctx.cl_read()
        return (got, also(ctx)) if also else got


def _flat(lists, W):
    return [w for wl in lists for w in (range(W) if wl is None else wl)]


# ---- 1. random configurations in a box of unequal sides -----------------------------------------------------------------
# (Np = 1 is not a case: pigs_ctx_create refuses Np < 2, so no context reaches pigs_cl_init with one particle.)
@pytest.mark.parametrize("Np", [2, 3, 64, 65, 257, 300])
@pytest.mark.parametrize("dim", [1, 2, 3])
def test_matches_numpy(gpu_lib, dim, Np):
    """Windows 0, 2 and Nb on one context (cl_init again resizes and zeroes); three walkers, the list split over three
    launches, walker 1 listed in two of them."""
    Nb, W = 3, 3
    cfg = _cfg(dim, Np, Nb)
    L = cfg.Lbox[:dim]
    rc = cn.threshold_rc(dim, DENSITY[dim], L)
    P = cn.random_paths(W, 2 * Nb + 1, Np, L, np.random.default_rng(100 * dim + Np))
    lists = [[2, 1], [0], [1]]
    VT, WF = gpu_lib.build_tables(cfg)
    with gpu_lib.PigsContext(cfg, VT, WF, n_walkers=W) as ctx:
        ctx.upload_all(P)
        for window in (0, 2, Nb):
            exp = cn.Window(P, Nb, window, L, rc).expected(_flat(lists, W))
            if window == Nb:
                tot, s = exp["nsize"].sum(axis=0), np.arange(1, Np + 1)
                assert exp["nbond"].sum() > 0
                if Np >= 64:
                    assert np.count_nonzero(tot) >= 3 and tot[0] > 0, "the input has no spread of sizes"
                if Np >= 257:
                    assert np.any(tot[64:] > 0), "the input has no cluster beyond 64 particles"
                assert np.array_equal((s * exp["nsize"]).sum(axis=1), Np * exp["samples"])
            ctx.cl_init(rc, window)
            for wl in lists:
                ctx.cl_accumulate(wl)
            got = ctx.cl_read()
            assert got["window"] == window and got["samples"].tolist() == [2 * window + 1, 2 * (2 * window + 1), 2 * window + 1]
            _assert_same(got, exp, f"dim {dim} Np {Np} window {window}")


# ---- 2. hand-built slices -----------------------------------------------------------------------------------------------
CHAIN_L = [600.0, 8.0, 8.0]


def _one_slice(gpu_lib, X, Lbox, rc):
    """X as the middle slice of one walker (window 0): (got, expected, the restatement's labels)."""
    dim, Np = X.shape[1], X.shape[0]
    cfg = _cfg(dim, Np, 1, Lbox=list(Lbox))
    P = cn.as_paths(X, 3)
    win = cn.Window(P, 1, 0, Lbox, rc)
    got = _run(gpu_lib, cfg, P, rc, 0, [None], also=lambda ctx: ctx.cl_sweeps())
    return got[0], win.expected([0]), win.sums(0)[0][4], got[1]


@pytest.mark.parametrize("order", ["ascending", "shuffled", "ends"])
@pytest.mark.parametrize("cut", [False, True])
def test_chain_of_300(gpu_lib, order, cut):
    """300 particles on a line at 0.9 rc, the indices ascending, shuffled, or alternately from both ends: one cluster of
    300 whatever the order; with one spacing of 1.1 rc, two."""
    n, rc = 300, 1.0
    idx = {"ascending": np.arange(n), "shuffled": np.random.default_rng(300).permutation(n), "ends": cn.order_both_ends(n)}[order]
    sp = np.full(n - 1, 0.9 * rc)
    if cut:
        sp[110] = 1.1 * rc
    X = cn.chain(n, sp, idx, origin=[-140.0, 1.0, -2.0])
    got, exp, label, sweeps = _one_slice(gpu_lib, X, CHAIN_L, rc)
    if cut:
        assert sorted(np.bincount(label)[np.bincount(label) > 0].tolist()) == [111, 189] and exp["nbond"][0] == n - 2
    else:
        assert not np.any(label) and exp["nsize"][0, n - 1] == 1 and exp["nbond"][0] == n - 1
    _assert_same(got, exp, f"chain {order} cut {cut}")
    print(f"chain {order} cut {cut}: {sweeps} sweeps")
    assert 1 <= sweeps <= n + 1


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_pair_through_the_periodic_image(gpu_lib, axis):
    L = np.array([8.0, 16.0, 4.0])
    X = np.zeros((3, 3))
    X[0, axis], X[1, axis] = 0.5 * L[axis] - 0.25, -0.5 * L[axis] + 0.25
    X[2] = 0.25 * L
    got, exp, label, _ = _one_slice(gpu_lib, X, L, 0.75)
    assert label.tolist() == [0, 0, 2] and exp["nbond"][0] == 1 and abs(X[0, axis] - X[1, axis]) > 0.75
    _assert_same(got, exp, f"image {axis}")
    assert got["rg2"][0, 1] == 0.25 / 4.0


def test_touching_pair_and_coincident_pair(gpu_lib):
    """r2 == rc2 exactly is no bond, nextafter(rc) is one; a coincident pair is no bond."""
    L = [8.0, 16.0, 4.0]
    X = np.array([[1.0, 0.0, 0.0], [1.5, 0.0, 0.0], [-2.0, 3.0, 1.0], [-2.0, 3.0, 1.0]])
    got, exp, label, _ = _one_slice(gpu_lib, X, L, 0.5)
    assert label.tolist() == [0, 1, 2, 3] and exp["nbond"][0] == 0
    _assert_same(got, exp, "r2 == rc2")
    assert got["nsize"][0].tolist() == [4, 0, 0, 0]
    got, exp, label, _ = _one_slice(gpu_lib, X, L, float(np.nextafter(0.5, np.inf)))
    assert label.tolist() == [0, 0, 2, 3] and exp["nbond"][0] == 1
    _assert_same(got, exp, "nextafter(rc)")
    assert got["nsize"][0].tolist() == [2, 1, 0, 0] and got["nlarge"][0].tolist() == [0, 1, 0, 0]


def test_two_equal_clusters_with_interleaved_indices(gpu_lib):
    """Even indices form one triangle, odd ones another of another shape: G_slice[3] is g(root 0) + g(root 1) in that order."""
    X = np.zeros((6, 2))
    X[0::2] = [[0.0, 0.0], [0.3, 0.0], [0.0, 0.4]]
    X[1::2] = [[4.0, 4.0], [4.1, 4.0], [4.0, 4.7]]
    got, exp, label, _ = _one_slice(gpu_lib, X, [16.0, 12.0], 0.75)
    assert label.tolist() == [0, 1, 0, 1, 0, 1] and exp["nsize"][0, 2] == 2 and exp["terms"][0, 2] == 1
    g = [cn.slice_sums(X[k::2], [16.0, 12.0], 0.75)[3][2] for k in (0, 1)]
    assert g[0] != g[1] and exp["rg2"][0, 2] == g[0] + g[1]
    _assert_same(got, exp, "interleaved")
    assert got["rg2"][0, 2] == g[0] + g[1]


def test_cluster_across_the_mask_words(gpu_lib):
    """One cluster of exactly the particles 63, 64, 255, 256 of 300, every other particle single."""
    n, rc = 300, 0.5
    X = np.zeros((n, 3))
    X[:, 0] = -290.0 + 1.9 * np.arange(n)
    X[[63, 64, 255, 256]] = [[295.0, 2.0, 1.0], [295.4, 2.0, 1.0], [295.4, 2.4, 1.0], [295.4, 2.4, 1.4]]
    got, exp, label, _ = _one_slice(gpu_lib, X, CHAIN_L, rc)
    want = np.arange(n)
    want[[64, 255, 256]] = 63
    assert np.array_equal(label, want) and exp["nbond"][0] == 3
    _assert_same(got, exp, "63, 64, 255, 256")
    assert got["nsize"][0, 0] == n - 4 and got["nsize"][0, 3] == 1 and got["nlarge"][0, 3] == 1


# ---- 3. both adjacency forms ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Np", [ADJ_MAX, ADJ_MAX + 1])
def test_both_adjacency_forms(gpu_lib, Np):
    """The bit rows in LDS up to kClAdjNpMax particles, the distances of every sweep beyond: one walker, window 0."""
    assert ADJ_MAX == 256
    cfg = _cfg(3, Np, 1)
    rc = cn.threshold_rc(3, DENSITY[3], cfg.Lbox)
    P = cn.random_paths(1, 3, Np, cfg.Lbox, np.random.default_rng(Np))
    exp = cn.Window(P, 1, 0, cfg.Lbox, rc).expected([0])
    assert exp["nbond"][0] > 0 and np.count_nonzero(exp["nsize"][0]) >= 3 and np.any(exp["nsize"][0, 64:] > 0)
    _assert_same(_run(gpu_lib, cfg, P, rc, 0, [None]), exp, f"form at Np {Np}")


# ---- 4. determinism ---------------------------------------------------------------------------------------------------
def _small():
    cfg = _cfg(3, 70, 3)
    return cfg, cn.random_paths(3, 7, 70, cfg.Lbox, np.random.default_rng(70)), cn.threshold_rc(3, DENSITY[3], cfg.Lbox)


def _same(a, b, what=""):
    for k in INTS:
        assert np.array_equal(a[k], b[k]), (what, k)
    assert same_bits(a["rg2"], b["rg2"]), (what, "rg2")


def test_list_splits_give_the_same_bits(gpu_lib):
    cfg, P, rc = _small()
    whole = _run(gpu_lib, cfg, P, rc, 2, [None])
    _same(_run(gpu_lib, cfg, P, rc, 2, [[2], [1], [0]]), whole, "one by one")
    _same(_run(gpu_lib, cfg, P, rc, 2, [[1, 0], [2]]), whole, "two and one")
    exp = cn.Window(P, 3, 2, cfg.Lbox, rc).expected(range(3))
    assert np.any(exp["terms"] > 1)                                     # elements of several terms: an order to keep
    _assert_same(whole, exp, "whole")


def test_scratch_budget_and_reset_mask(gpu_lib):
    """A budget of 1 MiB holds fewer walkers than the list: more launches, the same bits.  Then the per-walker reset."""
    Np, Nb, W = 300, 3, 70
    cfg = _cfg(2, Np, Nb)
    L = cfg.Lbox[:2]
    rc = cn.threshold_rc(2, DENSITY[2], L)
    P = np.broadcast_to(cn.random_paths(2, 2 * Nb + 1, Np, L, np.random.default_rng(5))[np.arange(W) % 2], (W, 7, Np, 2)).copy()
    assert (1 << 20) // (8 * 7 * Np) == 62 < W
    VT, WF = gpu_lib.build_tables(cfg)
    with gpu_lib.PigsContext(cfg, VT, WF, n_walkers=W) as ctx:
        ctx.upload_all(P)
        ctx.cl_init(rc, Nb)
        ctx.cl_accumulate()
        whole = ctx.cl_read()
        ctx.set_tuning("cl_scratch_mib", 1)
        ctx.cl_init(rc, Nb)
        ctx.cl_accumulate()
        split = ctx.cl_read(reset=[w == 1 for w in range(W)])
        again = ctx.cl_read()
        ARG = ST["PIGS_ERR_ARG"]
        assert ctx.L.pigs_set_tuning(ctx.h, b"cl_scratch_mib", 0) == ARG and ctx.L.pigs_set_tuning(ctx.h, b"cl_scratch_mib", 2049) == ARG
    _same(split, whole, "budget")
    exp = cn.Window(P[:2], Nb, Nb, L, rc).expected([0, 1])
    for k in INTS + ("rg2", "terms"):
        exp[k] = exp[k][np.arange(W) % 2]
    _assert_same(whole, exp, "budget")
    keep = np.arange(W) != 1
    for k in INTS + ("rg2",):
        assert np.array_equal(again[k][keep], split[k][keep]) and not np.any(again[k][1]), k


# ---- 5. refusals and statuses -----------------------------------------------------------------------------------------
def test_status_codes(gpu_lib):
    Nb = 3
    ARG, OK, UNS = ST["PIGS_ERR_ARG"], ST["PIGS_OK"], ST["PIGS_ERR_UNSUPPORTED"]
    cfg = _cfg(2, 30, Nb)
    half = 0.5 * min(cfg.Lbox[:2])
    VT, WF = gpu_lib.build_tables(cfg)
    with gpu_lib.PigsContext(cfg, VT, WF, n_walkers=2) as ctx:
        init = lambda rc, window: ctx.L.pigs_cl_init(ctx.h, C.c_double(rc), window)
        assert ctx.L.pigs_cl_accumulate(ctx.h, 1, None) == ARG              # before init
        with pytest.raises(gpu_lib.PigsError):
            ctx.cl_read()
        d, l = np.zeros(60), np.zeros(60, np.int64)
        dp, lp = d.ctypes.data_as(C.POINTER(C.c_double)), l.ctypes.data_as(C.POINTER(C.c_int64))
        assert ctx.L.pigs_cl_read(ctx.h, lp, lp, lp, lp, dp, None) == ARG
        sw = C.c_int32(0)
        assert ctx.L.pigs_cl_sweeps(ctx.h, C.byref(sw)) == ARG
        for args in ((0.0, 0), (-1.0, 0), (float("nan"), 0), (float("inf"), 0), (float(np.nextafter(half, np.inf)), 0),
                     (1.0, -1), (1.0, Nb + 1)):
            assert init(*args) == ARG, args
            assert ctx.L.pigs_cl_accumulate(ctx.h, 1, None) == ARG
        assert init(half, 0) == OK and init(1.0, Nb) == OK
        assert ctx.L.pigs_cl_accumulate(ctx.h, -1, None) == ARG
        assert ctx.L.pigs_cl_accumulate(ctx.h, 1, np.array([2], np.int32).ctypes.data_as(_ip)) == ARG
        assert ctx.L.pigs_cl_accumulate(ctx.h, 1, np.array([-1], np.int32).ctypes.data_as(_ip)) == ARG
        assert ctx.L.pigs_cl_accumulate(ctx.h, 0, None) == OK
        assert ctx.L.pigs_cl_read(ctx.h, lp, lp, lp, lp, None, None) == ARG
        ctx.sync()
        # Np above the limit: the constant of the header, of the library and of the Python layer, and the check that
        # PigsContext.cl_init makes on the host before the library is asked (no context of that size is allocated)
        limit = int(re.search(r"#define PIGS_CL_NP_MAX (\d+)", _header()).group(1))
        assert ctx.L.pigs_cl_np_max() == limit == api.CL_NP_MAX
        import types
        big = types.SimpleNamespace(cfg=types.SimpleNamespace(Np=limit + 1), L=None, h=None)
        with pytest.raises(gpu_lib.PigsError, match="Np"):
            gpu_lib.PigsContext.cl_init(big, 1.0, 0)
    tcfg = SystemConfig(dim=2, Np=6, Nb=2, trap=True, a_ho=[1.0, 1.3], Nmax=2000, Rm=1.2, dt=0.01)
    VT, WF = gpu_lib.build_tables(tcfg)
    with gpu_lib.PigsContext(tcfg, VT, WF, n_walkers=1) as ctx:
        assert ctx.L.pigs_cl_init(ctx.h, C.c_double(0.5), 0) == UNS
        assert ctx.L.pigs_cl_accumulate(ctx.h, 1, None) == ARG
        ctx.sync()


# ---- 6. beside the others ---------------------------------------------------------------------------------------------
def test_interleaved_with_bop_and_sf(gpu_lib):
    """pigs_bop_accumulate and pigs_sf_accumulate between two pigs_cl_accumulate on one context: each family keeps the
    bits it has alone."""
    cfg, P, rc = _small()
    VT, WF = gpu_lib.build_tables(cfg)

    def run(cl, others):
        with gpu_lib.PigsContext(cfg, VT, WF, n_walkers=3) as ctx:
            ctx.upload_all(P)
            if cl:
                ctx.cl_init(rc, 2)
            if others:
                ctx.bop_init(rc, 2, 20, 8, 0.25)
                ctx.sf_init(4, 2)
            for _ in range(2):
                if cl:
                    ctx.cl_accumulate()
                if others:
                    ctx.bop_accumulate([2, 0])
                    ctx.sf_accumulate([1])
            return (ctx.cl_read() if cl else None), ((ctx.bop_read(), ctx.sf_read()) if others else None)

    cl_alone, _ = run(True, False)
    _, (bop_alone, sf_alone) = run(False, True)
    cl_both, (bop_both, sf_both) = run(True, True)
    _same(cl_both, cl_alone)
    assert cl_both["samples"].tolist() == [10, 10, 10] and cl_both["nbond"].min() > 0
    for a, b in ((bop_alone, bop_both), (sf_alone, sf_both)):
        for k in a:
            if isinstance(a[k], np.ndarray):
                assert same_bits(a[k], b[k]) if a[k].dtype == np.float64 else np.array_equal(a[k], b[k]), k


# ---- 7. the front end ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def exe(gpu_lib):
    import subprocess
    host = os.path.join(ROOT, "pathintegralgroundstate_amd", "host")
    subprocess.check_call(["make", "-s", "-C", host])
    return os.path.join(host, "pigs_vpi")


def test_front_end_two_blocks_three_steps(gpu_lib, oracle, exe, tmp_path):
    """he4_cworm0 (2D, periodic, nine particles), 2 blocks x 3 steps, two walkers, clusters = T over a window of 2: every
    file of the run without the key byte for byte; the two new files of every walker against a replay of the run's chains
    through PigsContext.cl_* and normalize_cl."""
    from test_cl_host import check_files
    from test_gpu_front_end_blocks import _input, _run as run_vpi, replay
    run, W, Nblock, Nstep, window = "he4_cworm0", 2, 2, 3, 2
    txt, cfg = _input(run, Nblock, Nstep)
    assert not cfg.trap and cfg.Nb >= window
    rc = 0.6 * cfg.rcut
    key = f", clusters = T, cl_rc = {rc!r}, cl_window = {window}"
    rep = replay(gpu_lib, oracle, cfg, W, Nblock, Nstep)
    VT, WF = gpu_lib.build_tables(cfg)
    blocks = []
    with gpu_lib.PigsContext(cfg, VT, WF, n_walkers=W) as ctx:
        ctx.cl_init(rc, window)
        for b in range(Nblock):
            for t in range(b * Nstep, (b + 1) * Nstep):
                ctx.upload_all(rep["snaps"][t])
                wl = np.nonzero(rep["diag"][t])[0]
                if len(wl):
                    ctx.cl_accumulate(wl)
            blocks.append(ctx.cl_read(reset=True))
    counted = np.stack([b["samples"] > 0 for b in blocks], axis=1)           # [W, Nblock]
    assert counted.any() and sum(int(b["nbond"].sum()) for b in blocks) > 0
    assert sum(int(b["nsize"][:, 0].sum()) for b in blocks) > 0             # singles and bonded particles: a radius that tells
    plain, on = str(tmp_path / "plain"), str(tmp_path / "on")
    os.makedirs(plain), os.makedirs(on)
    run_vpi(exe, txt + f"&gpu\n n_walkers = {W}\n/\n", plain)
    out = run_vpi(exe, txt + f"&gpu\n n_walkers = {W}{key}\n/\n", on)
    assert "Clusters" in out and "clus_vpi.out" in out
    old = sorted(os.listdir(plain))
    new = sorted(set(os.listdir(on)) - set(old))
    assert sorted(f for f in new if ".w" not in f) == ["clus_vpi.out", "clusblk_vpi.out"], new
    assert len(new) == 2 + 2 * W, new
    for f in old:
        if f not in ("stdout.txt", "vpi.in"):
            assert open(os.path.join(plain, f), "rb").read() == open(os.path.join(on, f), "rb").read(), f
    names = sorted(f for f in new if re.fullmatch(r"clus_vpi\.w\d+\.out", f))
    assert len(names) == W
    checked = 0
    for w, fc in enumerate(names):
        bs = [b for b in range(Nblock) if counted[w, b]]
        if not bs:
            continue
        mine = [normalize_cl({k: v[w] for k, v in blocks[b].items() if k != "window"}, cfg.Np) for b in bs]
        check_files(os.path.join(on, fc), os.path.join(on, fc.replace("clus_", "clusblk_")), mine, cfg.Np,
                    block_ids=[b + 1 for b in bs])
        checked += 1
    assert checked > 0
