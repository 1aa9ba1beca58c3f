"""The triplet counts on the MI355X (pigs_g3_*, pigs_g3.hip) through the C ABI, against the numpy restatement in
tests/g3_numpy.py (pinned to a literal triple loop and to identities by tests/test_g3_numpy_host.py).  Every count is an
integer: every comparison is exact equality over all elements.

Shapes: Np = 2 (no triplet), 3 (one per vertex), 4, 63/64/65 (a wave's partner chunk), 256/257 (four chunks and one
partner more) and 300, in 2D and 3D with the radius at half the box, on a grid of Nr = 6, Na = 5 so that every diagonal
leg pair lo = hi and every angle bin holds counts, and in both kernel forms (tuning key g3_form) beside the automatic
choice.  The large systems run one slice of two walkers, the small ones a window of three slices."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import block_stats_numpy as bs
import g3_numpy
from conftest import ROOT
from g3_numpy import Window
from pathintegralgroundstate_amd import SystemConfig

pytestmark = pytest.mark.gpu
DENSITY = {2: 0.25, 3: 0.365}
FORMS = (0, 1, -1)
WAVES = 4                                                           # waves of a workgroup, each with a leg list


def _header():
    return open(os.path.join(ROOT, "include", "pigs_hip.h")).read()


ST = {k: int(v) for k, v in re.findall(r"^\s*(PIGS_\w+)\s*=\s*(-?\d+)", _header(), flags=re.M)}


def _lds_budget():
    """kG3LdsBudget of pigs_kernels.h, and the same number in the header's formulas."""
    txt = open(os.path.join(ROOT, "pathintegralgroundstate_amd", "csrc", "pigs_kernels.h")).read()
    a, b = re.search(r"constexpr\s+size_t\s+kG3LdsBudget\s*=\s*(\d+)\s*\*\s*(\d+)\s*;", txt).groups()
    n = int(a) * int(b)
    assert re.search(r"constexpr\s+int\s+kG3Waves\s*=\s*%d\s*;" % WAVES, txt)
    assert f"8 dim Np + 4 Np (8 (dim + 1) + 4) > {n}" in _header()
    assert f"8 dim Np + 4 Np (8 (dim + 1) + 4) + 4 (Nr(Nr+1)/2 Na + Nr) <= {n}" in _header()
    return n


LDS = _lds_budget()


def _base(dim, Np):
    return 8 * dim * Np + WAVES * Np * (8 * (dim + 1) + 4)


def _fits(dim, Np, Nr, Na):
    return _base(dim, Np) + 4 * (Nr * (Nr + 1) // 2 * Na + Nr) <= LDS and Np * (Np - 1) * (Np - 2) // 2 <= 2 ** 32 - 1


def _cfg(dim, Np, Nb, **kw):
    return SystemConfig(dim=dim, Np=Np, Nb=Nb, density=DENSITY[dim], **kw)


def _random_paths(cfg, W, rng, scale=0.5):
    L = np.asarray(cfg.Lbox[:cfg.dim])
    return rng.uniform(-scale, scale, (W,) + tuple(cfg.path_shape)) * L


def _half(cfg):
    return 0.5 * min(cfg.Lbox[:cfg.dim])


def _same(got, exp, what):
    for k in ("samples", "pair", "trip"):
        assert got[k].dtype == np.int64 and got[k].shape == exp[k].shape, (what, k, got[k].shape, exp[k].shape)
        assert np.array_equal(got[k], exp[k]), (what, k, int(np.abs(got[k] - exp[k]).sum()))


def _each_form(ctx, cfg, Nr, Na):
    """Sets every form in turn; a forced LDS form that does not fit is refused at the accumulate and skipped."""
    for form in FORMS:
        ctx.set_tuning("g3_form", form)
        if form == 1 and not _fits(cfg.dim, cfg.Np, Nr, Na):
            assert ctx.L.pigs_g3_accumulate(ctx.h, ctx.n_walkers, None) == ST["PIGS_ERR_ARG"]
            assert not ctx.g3_read()["samples"].any()                   # nothing was queued
            continue
        yield form
    ctx.set_tuning("g3_form", -1)


def _compare(ctx, cfg, win, window, Nr, rbin, Na, what, walkers=None):
    """init, one accumulate per form, each against the restatement (and so the forms against each other bit for bit)."""
    wl = range(ctx.n_walkers) if walkers is None else walkers
    exp = win.expected(wl, Nr, rbin, Na)
    ctx.g3_init(Nr, rbin, Na, window)
    forms = []
    for form in _each_form(ctx, cfg, Nr, Na):
        ctx.g3_accumulate(walkers)
        got = ctx.g3_read(reset=True)
        _same(got, exp, f"{what} window {window} Nr {Nr} Na {Na} form {form}")
        forms.append(form)
    return exp, forms


# ---- 1. against the restatement on random in-box worldlines -----------------------------------------------------------
@pytest.mark.parametrize("Np", [2, 3, 4, 63, 64, 65, 256, 257, 300])
@pytest.mark.parametrize("dim", [2, 3])
def test_matches_numpy_on_uploaded_worldlines(gpu_lib, dim, Np):
    W, Nr, Na = 2, 6, 5
    Nb, window = (2, 1) if Np <= 65 else (1, 0)
    cfg = _cfg(dim, Np, Nb)
    VT, WF = gpu_lib.build_tables(cfg)
    # a third of the particles anywhere in the box, a third in its central quarter and a third in its central tenth: the
    # innermost leg pairs hold counts too
    P = _random_paths(cfg, W, np.random.default_rng(1000 * dim + Np)) * np.array([1.0, 0.5, 0.2])[np.arange(Np) % 3, None]
    rbin = _half(cfg) / Nr                                              # rmax at half the box
    win = Window(P, Nb, window, cfg.Lbox)
    with gpu_lib.PigsContext(cfg, VT, WF, n_walkers=W) as ctx:
        ctx.upload_all(P)
        exp, forms = _compare(ctx, cfg, win, window, Nr, rbin, Na, f"dim {dim} Np {Np}")
    assert forms == list(FORMS)                                         # this grid fits the LDS at every Np here
    ns = 2 * window + 1
    if Np == 2:
        assert not exp["trip"].any() and exp["pair"].sum() > 0
    elif Np == 3:
        # at most one pair of legs per vertex, and exactly one wherever both partners are within the radius
        assert 0 < exp["trip"].sum() <= W * ns * 3
    if Np >= 63:
        diag = g3_numpy.packed_index(np.arange(Nr), np.arange(Nr), Nr)
        assert np.all(exp["trip"].sum(axis=0)[diag].sum(axis=1) > 0), "an empty diagonal leg pair"
        assert np.all(exp["trip"].sum(axis=(0, 1)) > 0) and np.all(exp["pair"].sum(axis=0) > 0), "an empty bin"


@pytest.mark.parametrize("dim,Np", [(2, 5), (3, 65)])
def test_grid_just_past_the_lds_budget(gpu_lib, dim, Np):
    """The largest Na whose counters still sit in LDS beside the slice and the leg lists, and the next one, which takes the
    global form automatically and refuses form 1."""
    W, Nb, window, Nr = 2, 1, 1, 40
    cfg = _cfg(dim, Np, Nb)
    pairs = Nr * (Nr + 1) // 2
    last = ((LDS - _base(dim, Np)) // 4 - Nr) // pairs
    assert _fits(dim, Np, Nr, last) and not _fits(dim, Np, Nr, last + 1) and last + 1 <= 1024
    VT, WF = gpu_lib.build_tables(cfg)
    P = _random_paths(cfg, W, np.random.default_rng(dim + Np))
    win = Window(P, Nb, window, cfg.Lbox)
    with gpu_lib.PigsContext(cfg, VT, WF, n_walkers=W) as ctx:
        ctx.upload_all(P)
        _, forms = _compare(ctx, cfg, win, window, Nr, _half(cfg) / Nr, last, f"threshold dim {dim}")
        assert forms == [0, 1, -1]
        _, forms = _compare(ctx, cfg, win, window, Nr, _half(cfg) / Nr, last + 1, f"past the threshold dim {dim}")
        assert forms == [0, -1]                                         # form 1 was refused, the automatic form ran


# ---- 2. edges -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [2, 3])
def test_constructed_edge_inputs(gpu_lib, dim):
    """Box of side 16 with Np = 64, rmax = 2 on Nr = 8 bins of 1/4, coordinates multiples of 1/8: every u is exact.
    Cluster A around the origin: a partner at exactly rmax (dropped) and one at rmax - 1/8 (kept), two coincident
    particles (no leg between them), three collinear particles (cos = +1 from the end, -1 from the middle).  Cluster B far
    away: two particles with exactly one leg each.  Walker 1 has a NaN and an Inf coordinate."""
    Np = 64
    cfg = SystemConfig(dim=dim, Np=Np, Nb=1, density=Np / 16.0 ** dim, Lbox=[16.0] * dim)
    assert list(cfg.Lbox[:dim]) == [16.0] * dim
    Nr, rbin, Na, W, window = 8, 0.25, 4, 2, 1
    X = np.zeros((Np, dim))
    # the rest sit on the line x = 5 (more than rmax from both clusters, also round the box), a quarter apart in y
    X[:, 0] = 5.0
    X[:, 1] = -7.75 + 0.25 * np.arange(Np)
    X[0] = 0.0                                                          # the vertex
    X[1] = 0.0; X[1, 0] = 2.0                                           # at exactly rmax: u = 8 = Nr, dropped
    X[2] = 0.0; X[2, 0] = -1.875                                        # just inside: bin 7
    X[3] = 0.0                                                          # coincides with the vertex
    X[4] = 0.0; X[4, 1] = 0.5                                           # 0, 4, 5 collinear along y
    X[5] = 0.0; X[5, 1] = 1.0
    X[6] = 0.0; X[6, 0] = -5.0; X[6, 1] = -6.0                          # cluster B: 6 and 7 see only each other
    X[7] = X[6]; X[7, 1] = -5.5
    P = np.broadcast_to(X, (W, 3, Np, dim)).copy()
    P[1, 1, 9, 0] = np.nan
    P[1, 1, 10, dim - 1] = np.inf
    win = Window(P, 1, window, cfg.Lbox)
    # what the restatement says of the constructed cases, before the device is asked
    d, s, b = g3_numpy.legs(X, 0, cfg.Lbox, Nr, rbin)
    assert sorted(b.tolist()) == [2, 4, 7]
    t0, _, nleg = g3_numpy.slice_counts(X, cfg.Lbox, Nr, rbin, Na)
    assert nleg[:8].tolist() == [3, 0, 3, 3, 4, 3, 1, 1]
    p24 = g3_numpy.packed_index(2, 4, Nr)
    assert t0[p24, Na - 1] >= 2 and t0[g3_numpy.packed_index(2, 2, Nr), 0] >= 1      # cos = +1 and cos = -1
    VT, WF = gpu_lib.build_tables(cfg)
    with gpu_lib.PigsContext(cfg, VT, WF, n_walkers=W) as ctx:
        ctx.upload_all(P)
        exp, _ = _compare(ctx, cfg, win, window, Nr, rbin, Na, f"edges dim {dim}")
    assert exp["trip"][1].sum() < exp["trip"][0].sum()                  # the NaN and the Inf dropped legs


@pytest.mark.parametrize("dim", [2, 3])
def test_box_with_unequal_sides(gpu_lib, dim):
    Np, Nb, W, window, Nr, Na = 65, 2, 2, 2, 6, 5
    L = (Np / DENSITY[dim]) ** (1.0 / dim)
    cfg = _cfg(dim, Np, Nb, Lbox=[0.8 * L, 1.25 * L] if dim == 2 else [0.8 * L, 1.25 * L, L])
    VT, WF = gpu_lib.build_tables(cfg)
    P = _random_paths(cfg, W, np.random.default_rng(77 + dim))
    with gpu_lib.PigsContext(cfg, VT, WF, n_walkers=W) as ctx:
        ctx.upload_all(P)
        _compare(ctx, cfg, Window(P, Nb, window, cfg.Lbox), window, Nr, _half(cfg) / Nr, Na, f"unequal sides dim {dim}")
        # beyond half the SHORTEST side: refused, as pigs_bop_init refuses rnb
        assert ctx.L.pigs_g3_init(ctx.h, Nr, 1.01 * _half(cfg) / Nr, Na, 0) == ST["PIGS_ERR_ARG"]


# ---- 3. invariance --------------------------------------------------------------------------------------------------
def test_counts_do_not_depend_on_the_list_or_the_split(gpu_lib):
    """A list of 300 entries over 3 walkers of Np = 5 (two launches, split at 256), two calls, a reversed list, the reset
    mask, a second init and a fresh context."""
    W, Np, dim, Nb, window, Nr, Na = 3, 5, 3, 2, 2, 4, 3
    cfg = _cfg(dim, Np, Nb)
    VT, WF = gpu_lib.build_tables(cfg)
    P = _random_paths(cfg, W, np.random.default_rng(9))
    rbin = _half(cfg) / Nr
    win = Window(P, Nb, window, cfg.Lbox)
    long = [(7 * i) % W for i in range(300)]
    with gpu_lib.PigsContext(cfg, VT, WF, n_walkers=W) as ctx:
        ctx.upload_all(P)
        ctx.g3_init(Nr, rbin, Na, window)
        for form in _each_form(ctx, cfg, Nr, Na):
            ctx.g3_accumulate(long)
            whole = ctx.g3_read(reset=True)
            _same(whole, win.expected(long, Nr, rbin, Na), f"300 entries form {form}")
            assert whole["trip"].sum() > 0
            ctx.g3_accumulate(long[:100])
            ctx.g3_accumulate(long[100:])
            _same(ctx.g3_read(reset=True), whole, "two calls")
            ctx.g3_accumulate(long[::-1])
            _same(ctx.g3_read(reset=True), whole, "reversed list")
            ctx.g3_accumulate()
            ctx.g3_accumulate([2, 2])
            thrice = ctx.g3_read()
            _same(thrice, win.expected([0, 1, 2, 2, 2], Nr, rbin, Na), "NULL list and a walker listed twice")
            # reset zeroes only the walkers named
            mask = np.zeros(W, np.int32)
            mask[1] = 1
            ctx.g3_read(reset=mask)
            after = ctx.g3_read(reset=True)
            assert after["samples"].tolist() == [1, 0, 3] and not after["trip"][1].any() and not after["pair"][1].any()
            assert np.array_equal(after["trip"][2], thrice["trip"][2]) and np.array_equal(after["pair"][0], thrice["pair"][0])
        # a second init resizes and zeroes, also with a call in flight
        ctx.g3_accumulate()
        ctx.g3_init(2, rbin, 7, 1)
        z = ctx.g3_read()
        assert z["trip"].shape == (W, 3, 7) and z["pair"].shape == (W, 2) and not any(z[k].any() for k in z)
        ctx.g3_accumulate([1])
        _same(ctx.g3_read(), Window(P, Nb, 1, cfg.Lbox).expected([1], 2, rbin, 7), "after re-init")
    # a fresh context with one walker: the same worldline, the same counts
    with gpu_lib.PigsContext(cfg, VT, WF, n_walkers=1) as one:
        one.upload_all(P[2:3])
        one.g3_init(Nr, rbin, Na, window)
        one.g3_accumulate()
        got = one.g3_read()
        e = win.expected([2], Nr, rbin, Na)
        for k in ("trip", "pair", "samples"):
            assert np.array_equal(got[k][0], e[k][2]), k


@pytest.mark.parametrize("dim,Np", [(2, 70), (3, 130)])
def test_pair_counts_equal_the_van_hove_lag_zero(gpu_lib, dim, Np):
    """One worldline without coincidences, rmax = rcut: `pair` is pigs_vh_*'s distinct histogram at lag 0 on the same grid
    and window."""
    W, Nb, window, Nr, Na = 2, 2, 2, 25, 3
    cfg = _cfg(dim, Np, Nb)
    assert cfg.rcut <= _half(cfg) * (1 + 1e-15)
    rbin = cfg.rcut / Nr
    VT, WF = gpu_lib.build_tables(cfg)
    P = _random_paths(cfg, W, np.random.default_rng(31 + dim))
    with gpu_lib.PigsContext(cfg, VT, WF, n_walkers=W) as ctx:
        ctx.upload_all(P)
        ctx.g3_init(Nr, rbin, Na, window)
        ctx.g3_accumulate()
        ctx.vh_init(0, window, Nr, rbin, 1, 1.0)
        ctx.vh_accumulate()
        g3, vh = ctx.g3_read(), ctx.vh_read()
    assert g3["pair"].sum() > 0 and np.array_equal(g3["pair"], vh["distinct"][:, 0])


# ---- 4. after the sampler ---------------------------------------------------------------------------------------------
RUNS = os.path.join(ROOT, "tests", "golden", "vpi_runs")


def _chain(gpu_lib, oracle, cfg, W, steps, g3=None):
    """`steps` MC steps of W chains as the front end starts them; g3 = (Nr, rbin, Na, window): an accumulate queued behind
    every step, with no synchronisation in between.  (worldlines after every step, final, g3_read)."""
    from oracle.pyoracle import System
    S = System(dim=cfg.dim, Np=cfg.Np, Nb=cfg.Nb, density=cfg.density, dt=cfg.dt, trap=cfg.trap, a_ho=cfg.a_ho,
               Lbox=cfg.Lbox, rcut=cfg.rcut)
    VT, WF = gpu_lib.build_tables(cfg)
    with gpu_lib.PigsContext(cfg, VT, WF, n_walkers=W) as ctx:
        ctx.sampler_init(CWorm=cfg.CWorm, swapping=cfg.swapping, Nobdm=cfg.Nobdm, Nbin=cfg.Nbin, Npw=cfg.Npw,
                         sampling=cfg.sampling)
        P0, xend = [], []
        for w in range(W):
            P, g = oracle.init_path(S, cfg.seed + w)
            P0.append(P)
            xend.append(np.stack([P[cfg.Nb, cfg.Np - 1], P[cfg.Nb, cfg.Np - 1]]))
            ctx.sampler_set_rng(w, g.mti, np.array(g.mt[:], np.uint32))
        ctx.upload_all(np.stack(P0))
        ctx.sampler_set_worm(np.zeros(W, np.int32), np.zeros(W, np.int32), np.stack(xend))
        snaps = []
        if g3 is not None:
            ctx.g3_init(*g3)
        for istep in range(1, steps + 1):
            ctx.sampler_step(istep)
            if g3 is not None:
                ctx.g3_accumulate()
            else:
                snaps.append(ctx.download_all())
        return snaps, ctx.download_all(), (ctx.g3_read() if g3 is not None else None)


def test_accumulate_behind_sampler_steps_with_swaps(gpu_lib, oracle):
    """he4_wormbusy_s7 (3D, worm and swap moves on): the counts queued behind every step are the restatement's on the
    worldlines a twin chain downloads after the same steps, and the family leaves the worldlines bit-identical."""
    cfg = SystemConfig.from_namelists(open(os.path.join(RUNS, "he4_wormbusy_s7", "vpi.in")).read())
    assert cfg.swapping and cfg.CWorm > 0 and not cfg.trap
    W, steps, Nr, Na, window = 3, 6, 5, 4, 1
    rbin = 0.6 * _half(cfg) / Nr
    snaps, final_plain, _ = _chain(gpu_lib, oracle, cfg, W, steps)
    _, final_g3, got = _chain(gpu_lib, oracle, cfg, W, steps, (Nr, rbin, Na, window))
    assert np.array_equal(final_plain, final_g3) and np.array_equal(final_plain, snaps[-1])
    exp = None
    for Pn in snaps:
        e = Window(Pn, cfg.Nb, window, cfg.Lbox).expected(range(W), Nr, rbin, Na)
        exp = e if exp is None else {k: exp[k] + e[k] for k in e}
    _same(got, exp, "behind sampler_step")
    assert got["trip"].sum() > 0


# ---- 5. refusals ----------------------------------------------------------------------------------------------------
def test_status_codes(gpu_lib):
    W, Nb = 2, 3
    ARG, OK, UNS = ST["PIGS_ERR_ARG"], ST["PIGS_OK"], ST["PIGS_ERR_UNSUPPORTED"]
    assert len({ARG, OK, UNS}) == 3
    cfg = _cfg(2, 30, Nb)
    half = _half(cfg)
    VT, WF = gpu_lib.build_tables(cfg)
    l = np.zeros(1 << 16, np.int64).ctypes.data_as(C.POINTER(C.c_int64))
    nan, inf = float("nan"), float("inf")
    with gpu_lib.PigsContext(cfg, VT, WF, n_walkers=W) as ctx:
        ctx.upload_all(_random_paths(cfg, W, np.random.default_rng(2)))
        init = lambda *a: ctx.L.pigs_g3_init(ctx.h, *a)
        with pytest.raises(gpu_lib.PigsError):
            ctx.g3_accumulate()
        with pytest.raises(gpu_lib.PigsError):
            ctx.g3_read()
        assert ctx.L.pigs_g3_accumulate(ctx.h, 1, None) == ARG and ctx.L.pigs_g3_read(ctx.h, l, l, l, None) == ARG
        for Nr, rbin, Na, window in ((0, 0.1, 5, 0), (-1, 0.1, 5, 0), (1025, 1e-6, 5, 0), (5, 0.1, 0, 0), (5, 0.1, -2, 0),
                                     (5, 0.1, 1025, 0), (5, 0.0, 5, 0), (5, -0.1, 5, 0), (5, nan, 5, 0), (5, inf, 5, 0),
                                     (5, 0.1, 5, -1), (5, 0.1, 5, Nb + 1),
                                     (5, 1.001 * half / 5, 5, 0),                       # rmax beyond half the side
                                     (1024, 1e-6, 1024, 0)):                            # over 2 GiB
            assert init(Nr, rbin, Na, window) == ARG, (Nr, rbin, Na, window)
            with pytest.raises(gpu_lib.PigsError):
                ctx.g3_init(Nr, rbin, Na, window)
        assert ctx.L.pigs_g3_accumulate(ctx.h, 1, None) == ARG             # init stays undone
        # the limits themselves are accepted
        assert init(1, 1e-300, 1, Nb) == OK and init(1024, 1e-6, 1, 0) == OK and init(7, half / 7, 1024, 0) == OK
        ctx.g3_init(5, half / 5, 4, Nb)
        for bad in ([2], [-1], [0, 2]):
            with pytest.raises(gpu_lib.PigsError):
                ctx.g3_accumulate(bad)
        assert ctx.L.pigs_g3_accumulate(ctx.h, -1, None) == ARG
        assert ctx.L.pigs_g3_read(ctx.h, None, l, l, None) == ARG and ctx.L.pigs_g3_read(ctx.h, l, None, l, None) == ARG
        assert ctx.L.pigs_set_tuning(ctx.h, b"g3_form", 2) == ARG and ctx.L.pigs_set_tuning(ctx.h, b"g3_form", -2) == ARG
        assert ctx.L.pigs_g3_accumulate(ctx.h, W, None) == OK
        assert ctx.g3_read()["samples"].tolist() == [1] * W               # the refused lists added nothing
    # the size limit: slice and leg lists against the budget, the formula of the header; Np = 512 is served
    top = LDS // (8 * 3 + WAVES * (8 * 4 + 4))
    assert top >= 512
    for Np, want in ((512, OK), (top, OK), (top + 1, ARG)):
        big = _cfg(3, Np, 1)
        assert (_base(3, Np) > LDS) == (want == ARG)
        VT, WF = gpu_lib.build_tables(big)
        with gpu_lib.PigsContext(big, VT, WF, n_walkers=1) as ctx:
            assert ctx.L.pigs_g3_init(ctx.h, 10, _half(big) / 10, 10, 0) == want, Np
            ctx.sync()
    # dim = 1 and trapped contexts: unsupported, a status of its own
    one = SystemConfig(dim=1, Np=6, Nb=2, density=0.2)
    tcfg = SystemConfig(dim=2, Np=6, Nb=2, trap=True, a_ho=[1.0, 1.3], Nmax=2000, Rm=1.2, dt=0.01)
    for c, word in ((one, "2D and 3D"), (tcfg, "periodic")):
        VT, WF = gpu_lib.build_tables(c)
        with gpu_lib.PigsContext(c, VT, WF, n_walkers=1) as ctx:
            assert ctx.L.pigs_g3_init(ctx.h, 5, 0.1, 5, 0) == UNS
            assert ctx.L.pigs_g3_accumulate(ctx.h, 1, None) == ARG            # still before init
            with pytest.raises(gpu_lib.PigsError, match=word):
                ctx.g3_init(5, 0.1, 5)
            ctx.sync()                                                        # the context still works


# ---- 6. the front end -------------------------------------------------------------------------------------------------
PRINT = 1.0000001e-9            # the files carry 10 significant digits


@pytest.fixture(scope="module")
def exe(gpu_lib):
    import subprocess
    host = os.path.join(ROOT, "pathintegralgroundstate_amd", "host")
    subprocess.check_call(["make", "-s", "-C", host])
    return os.path.join(host, "pigs_vpi")


def _check_table(path, lead, bv, counted, w, what):
    """One file (the columns `lead`, then mean and error) against the block values bv [W, Nblock, n]."""
    tab = np.loadtxt(path)
    assert tab.shape == (bv.shape[2], lead.shape[1] + 2), (what, tab.shape)
    assert np.allclose(tab[:, :lead.shape[1]], lead, rtol=PRINT, atol=1e-300)
    mean, err, nb = bs.walker_stats(bv, counted, w) if w is not None else bs.average_stats(bv, counted)
    assert nb == bv.shape[1]
    mtol = PRINT * np.abs(mean)
    assert np.all(np.abs(tab[:, -2] - mean) <= mtol), (what, np.abs(tab[:, -2] - mean).max())
    etol = np.sqrt(4.0 * np.abs(mean) * mtol) + PRINT * np.abs(err)
    nan = np.isnan(tab[:, -1])
    assert not np.any(nan & (err > etol)) and np.all(np.abs(tab[:, -1] - err)[~nan] <= etol[~nan]), what
    assert np.any(err > etol) and mean.any(), (what, "no well-conditioned error bar: the check has no teeth")


def test_front_end_two_walkers_three_blocks(gpu_lib, oracle, exe, tmp_path):
    """he4_cworm0 (2D, CWorm = 0: every step is a diagonal one) with two walkers, once plain and once with triplet = T:
    the old files byte for byte, g3_vpi.out / g3ang_vpi.out per walker and averaged against a replay of the run's chains
    through PigsContext.g3_*, normalize_g3 / bond_angle and the block statistics of tests/block_stats_numpy.py."""
    from pathintegralgroundstate_amd.profiles import bond_angle, normalize_g3
    from test_gpu_front_end_blocks import _input, _run as run_vpi, replay
    W, Nblock, Nstep, Nr, Na, window = 2, 3, 2, 4, 6, 1
    txt, cfg = _input("he4_cworm0", Nblock, Nstep)
    rmax = round(0.75 * cfg.rcut * 64.0) / 64.0                              # (exact in the namelist's decimal digits)
    key = f", triplet = T, g3_nr = {Nr}, g3_na = {Na}, g3_rmax = {rmax!r}, g3_window = {window}"
    plain, on = str(tmp_path / "plain"), str(tmp_path / "on")
    run_vpi(exe, txt + f"&gpu\n n_walkers = {W}\n/\n", plain)
    out = run_vpi(exe, txt + f"&gpu\n n_walkers = {W}{key}\n/\n", on)
    assert "Triplet" in out
    old = sorted(os.listdir(plain))
    new = sorted(set(os.listdir(on)) - set(old))
    assert sorted(f for f in new if ".w" not in f) == ["g3_vpi.out", "g3ang_vpi.out"] and len(new) == 2 + 2 * W, new
    for f in old:
        if f not in ("stdout.txt", "vpi.in"):
            assert open(os.path.join(plain, f), "rb").read() == open(os.path.join(on, f), "rb").read(), f
    rep = replay(gpu_lib, oracle, cfg, W, Nblock, Nstep)
    final = np.fromfile(os.path.join(on, "worldlines_final.bin")).reshape(rep["final"].shape)
    assert np.array_equal(final, rep["final"]) and rep["diag"].all()
    rbin = rmax / Nr
    VT, WF = gpu_lib.build_tables(cfg)
    npk = Nr * (Nr + 1) // 2
    G3 = np.zeros((W, Nblock, npk * Na))
    PA = np.zeros((W, Nblock, Na))
    with gpu_lib.PigsContext(cfg, VT, WF, n_walkers=W) as ctx:
        ctx.g3_init(Nr, rbin, Na, window)
        for b in range(Nblock):
            for P in rep["snaps"][b * Nstep:(b + 1) * Nstep]:
                ctx.upload_all(P)
                ctx.g3_accumulate()
            raw = ctx.g3_read(reset=True)
            n = normalize_g3(raw, cfg.Np, window, cfg.density, rbin, cfg.dim)
            G3[:, b] = n["g3"].reshape(W, -1)
            PA[:, b] = bond_angle(raw["trip"], Nr)
    assert not np.array_equal(G3[0, 0], G3[0, 1])                            # the blocks differ: the errors have teeth
    lead3 = np.stack([np.repeat(n["r"][n["lo"]], Na), np.repeat(n["r"][n["hi"]], Na), np.tile(n["cos"], npk)], axis=1)
    leada = n["cos"][:, None]
    counted = np.ones((W, Nblock), bool)
    per_walker = sorted(f for f in new if re.fullmatch(r"g3_vpi\.w\d+\.out", f))
    assert len(per_walker) == W
    for w, f in enumerate(per_walker):
        _check_table(os.path.join(on, f), lead3, G3, counted, w, f)
        _check_table(os.path.join(on, f.replace("g3_", "g3ang_")), leada, PA, counted, w, f.replace("g3_", "g3ang_"))
    _check_table(os.path.join(on, "g3_vpi.out"), lead3, G3, counted, None, "g3_vpi.out")
    _check_table(os.path.join(on, "g3ang_vpi.out"), leada, PA, counted, None, "g3ang_vpi.out")


@pytest.mark.parametrize("extra,word", [(", g3_rmax = 1.d3", "g3_rmax"), (", g3_na = 0", "g3_na"), (", g3_na = 1025", "g3_na")])
def test_front_end_refuses_bad_keys_before_any_gpu_work(gpu_lib, exe, tmp_path, extra, word):
    import subprocess
    from test_gpu_front_end_blocks import _input
    txt, _ = _input("he4_cworm0", 1, 1)
    wd = str(tmp_path)
    with open(os.path.join(wd, "vpi.in"), "w") as f:
        f.write(txt + f"&gpu\n triplet = T{extra}\n/\n")
    with open(os.path.join(wd, "vpi.in")) as fin:
        r = subprocess.run([exe], stdin=fin, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, cwd=wd, timeout=120)
    out = r.stdout.decode(errors="replace")
    assert r.returncode == 2 and "triplet" in out and word in out, out[-2000:]
    assert not os.path.exists(os.path.join(wd, "e_vpi.out"))
