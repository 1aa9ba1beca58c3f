"""The Axilrod-Teller-Muto three-body sums on the MI355X (pigs_atm_*, pigs_atm.hip), through the C ABI and the front end.

The expected sums come from the numpy restatement in tests/atm_numpy.py (the same IEEE operations per term; pinned to a
literal triple loop and to closed forms by tests/test_atm_numpy_host.py).  ntrip and samples are integers and must be
equal.  The bound on T per element is 1e-12 * Sum|t| from the numpy side: the project's kernel tolerance in
tests/test_gpu_tau.py's form; the terms have both signs, so a bound relative to T would be wrong.  With Np = 3 an element is
ONE term and must have the restatement's bits.  No comparison masks or skips elements.  The inputs are jittered lattices
(tau_numpy.lattice_paths; a third of a grid's sites for the first-shell radius): no pair comes near coincidence, which
every case asserts."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from atm_numpy import Window, pair_r2, slice_sums
from conftest import ROOT
from helpers import same_bits
from pathintegralgroundstate_amd import SystemConfig
from pathintegralgroundstate_amd.profiles import normalize_atm, pressure_atm
from tau_numpy import lattice_paths, min_max_distance

pytestmark = pytest.mark.gpu
DENSITY = {2: 0.25, 3: 0.365}
WAVES = 4                                                           # waves of a workgroup, each with a leg list


def _header():
    return open(os.path.join(ROOT, "include", "pigs_hip.h")).read()


ST = {k: int(v) for k, v in re.findall(r"^\s*(PIGS_\w+)\s*=\s*(-?\d+)", _header(), flags=re.M)}
assert ST["PIGS_OK"] == 0 and len({ST["PIGS_ERR_ARG"], ST["PIGS_ERR_HIP"], ST["PIGS_ERR_UNSUPPORTED"]}) == 3


def _lds_budget():
    """kAtmLdsBudget and kAtmLdsTail of pigs_kernels.h, and the same numbers in the header's formula."""
    txt = open(os.path.join(ROOT, "pathintegralgroundstate_amd", "csrc", "pigs_kernels.h")).read()
    a, b = re.search(r"constexpr\s+size_t\s+kAtmLdsBudget\s*=\s*(\d+)\s*\*\s*(\d+)\s*;", txt).groups()
    tail = int(re.search(r"constexpr\s+size_t\s+kAtmLdsTail\s*=\s*(\d+)\s*;", txt).group(1))
    assert re.search(r"constexpr\s+int\s+kAtmWaves\s*=\s*%d\s*;" % WAVES, txt)
    assert f"8 dim Np + 4 Np 8 (dim + 1) + {tail} > {int(a) * int(b)}" in _header()
    return int(a) * int(b), tail


LDS, TAIL = _lds_budget()


def _cfg(dim, Np, Nb, **kw):
    return SystemConfig(dim=dim, Np=Np, Nb=Nb, density=DENSITY[dim], **kw)


def _half(cfg):
    return 0.5 * min(cfg.Lbox[:cfg.dim])


def _paths(cfg, W, rng, scale=1.0):
    """Jittered lattice; scale < 1 draws it together about the origin (a cluster: every side of a few particles' triangles
    within half the box)."""
    P = lattice_paths(cfg, W, rng) * scale
    lo, _ = min_max_distance(P, cfg)
    n = int(np.ceil(cfg.Np ** (1.0 / cfg.dim) - 1e-9))
    assert lo > 0.6 * scale * min(cfg.Lbox[:cfg.dim]) / n, lo          # no pair comes near coincidence
    return P


def _dilute_paths(cfg, W, rng, fill=3):
    """Np of the about fill * Np sites of a grid, drawn at random and in random order, every bead with its own jitter of
    +-0.1 spacings: (paths, spacing).  The neighbourhoods differ from vertex to vertex, down to none."""
    dim, Np, M = cfg.dim, cfg.Np, 2 * cfg.Nb + 1
    n = int(np.ceil((fill * Np) ** (1.0 / dim) - 1e-9))
    L = np.asarray(cfg.Lbox[:dim], float)
    a = L / n
    sites = rng.choice(n ** dim, Np, replace=False)
    idx = np.stack(np.unravel_index(sites, (n,) * dim), axis=1).astype(float)
    P = (idx[None, None] + 0.5 + rng.uniform(-0.1, 0.1, (W, M, Np, dim))) * a - 0.5 * L
    P = P - L * np.floor((P + 0.5 * L) / L)
    lo, _ = min_max_distance(P, cfg)
    assert lo > 0.6 * a.min(), lo
    return P, float(a.min())


def _assert_same(got, exp, what):
    """samples and ntrip equal, T within 1e-12 Sum|t| in every element."""
    assert got["T"].shape == exp["T"].shape and got["T"].dtype == np.float64, (what, got["T"].shape)
    assert got["ntrip"].dtype == np.int64 and got["samples"].dtype == np.int64
    assert np.array_equal(got["samples"], exp["samples"]), (what, got["samples"])
    assert np.array_equal(got["ntrip"], exp["ntrip"]), (what, int(np.abs(got["ntrip"] - exp["ntrip"]).sum()))
    assert np.all(np.isfinite(exp["T"])), what
    bound = 1e-12 * exp["abs"]
    err = np.abs(got["T"] - exp["T"])
    with np.errstate(all="ignore"):
        worst = float(np.max(np.where(err == 0, 0.0, err / bound)))
    print(f"{what}: max |got-want|/bound = {worst:.3e} over {err.size} elements, {int(exp['ntrip'].sum())} triplets")
    assert np.all(np.isfinite(got["T"])) and np.all(err <= bound), (what, worst)


def _run_lists(gpu_lib, cfg, paths, rc, window, lists):
    VT, WF = gpu_lib.build_tables(cfg)
    with gpu_lib.PigsContext(cfg, VT, WF, n_walkers=paths.shape[0]) as ctx:
        ctx.upload_all(paths)
        ctx.atm_init(rc, window)
        for wl in lists:
            ctx.atm_accumulate(wl)
        return ctx.atm_read()


# ---- 1. against the numpy restatement -----------------------------------------------------------------------------------
_SHARED = {}


def _case(dim, Np, Nb):
    """The worldlines of a shape and the per-slice sums every window of it shares."""
    key = (dim, Np, Nb)
    if key not in _SHARED:
        cfg = _cfg(dim, Np, Nb)
        # (up to five particles: a cluster of half the lattice's spacing, so that their triangles lie within rc)
        _SHARED[key] = (cfg, _paths(cfg, 2, np.random.default_rng(1000 * dim + 10 * Np + Nb), 0.5 if Np <= 5 else 1.0), {})
    return _SHARED[key]


@pytest.mark.parametrize("full_window", [False, True])
@pytest.mark.parametrize("Nb", [1, 4])
@pytest.mark.parametrize("Np", [3, 4, 5, 64, 65, 129, 256, 257, 300])
@pytest.mark.parametrize("dim", [2, 3])
def test_matches_numpy(gpu_lib, dim, Np, Nb, full_window):
    """rc at half the box; window 0 and Nb.  Np = 3: one term per element, the restatement's bits."""
    cfg, P, slices = _case(dim, Np, Nb)
    window = Nb if full_window else 0
    rc = _half(cfg)
    exp = Window(P, Nb, window, cfg.Lbox, slices).expected(range(2), rc)
    got = _run_lists(gpu_lib, cfg, P, rc, window, [None])
    _assert_same(got, exp, f"dim {dim} Np {Np} Nb {Nb} window {window}")
    assert exp["ntrip"].min() >= 1
    if Np == 3:
        assert np.all(exp["ntrip"] == 1) and same_bits(got["T"], exp["T"])
    else:
        assert exp["ntrip"].min() > 1


@pytest.mark.parametrize("dim,Np", [(2, 65), (3, 300)])
def test_first_shell_radius(gpu_lib, dim, Np):
    """A third of a grid's sites filled, rc = 1.6 spacings (the first and second neighbours): many vertices have no leg
    j > i within rc or one, others a handful."""
    Nb, window = 2, 2
    cfg = _cfg(dim, Np, Nb)
    P, a = _dilute_paths(cfg, 2, np.random.default_rng(77 + dim))
    rc = 1.6 * a
    assert rc < 0.5 * _half(cfg)
    near = pair_r2(P[0, Nb], cfg.Lbox) <= rc * rc
    legs = np.array([near[i, i + 1:].sum() for i in range(Np)])
    assert (legs == 0).sum() >= Np // 16 and (legs == 1).sum() >= Np // 16 and (legs >= 2).sum() >= Np // 4, np.bincount(legs)
    exp = Window(P, Nb, window, cfg.Lbox).expected(range(2), rc)
    got = _run_lists(gpu_lib, cfg, P, rc, window, [None])
    _assert_same(got, exp, f"first shell dim {dim} Np {Np}")
    assert exp["ntrip"].min() > Np // 8


# ---- 2. edges ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [2, 3])
def test_triplet_whose_nearest_images_do_not_close(gpu_lib, dim):
    """Three particles on the x axis of a cubic box of side L, 0.4 L apart, rc = L/2: the sides are 0.4 L, 0.2 L (round
    the box) and 0.4 L.  The term is the isosceles triangle's, bit for bit the restatement's."""
    cfg = _cfg(dim, 3, 1)
    Lx = cfg.Lbox[0]
    X = np.zeros((3, dim))
    X[:, 0] = [-0.4 * Lx, 0.0, 0.4 * Lx]
    P = np.broadcast_to(X, (1, 3, 3, dim)).copy()
    rc = _half(cfg)
    exp = Window(P, 1, 1, cfg.Lbox).expected([0], rc)
    got = _run_lists(gpu_lib, cfg, P, rc, 1, [None])
    assert got["ntrip"].tolist() == [[1, 1, 1]] and np.array_equal(got["ntrip"], exp["ntrip"])
    assert same_bits(got["T"], exp["T"])
    a, b = 0.4 * Lx, 0.2 * Lx
    want = (1.0 + 3.0 * ((2 * a * a - b * b) / (2 * a * a)) * (b / (2 * a)) ** 2) / (a * a * b) ** 3
    collinear = -2.0 / (a * a * 2 * a) ** 3
    assert np.all(np.abs(got["T"] - want) <= 1e-13 * want) and want > 0 > collinear


@pytest.mark.parametrize("dim", [2, 3])
def test_box_with_unequal_sides(gpu_lib, dim):
    Np, Nb, window = 65, 2, 2
    L = (Np / DENSITY[dim]) ** (1.0 / dim)
    cfg = _cfg(dim, Np, Nb, Lbox=[0.8 * L, 1.25 * L] if dim == 2 else [0.8 * L, 1.25 * L, L])
    assert len(set(cfg.Lbox[:dim])) == dim and _half(cfg) == 0.5 * cfg.Lbox[0]
    P = _paths(cfg, 2, np.random.default_rng(70 + dim))
    rc = _half(cfg)
    exp = Window(P, Nb, window, cfg.Lbox).expected(range(2), rc)
    got = _run_lists(gpu_lib, cfg, P, rc, window, [None])
    _assert_same(got, exp, f"unequal sides dim {dim}")
    assert exp["ntrip"].min() > Np
    VT, WF = gpu_lib.build_tables(cfg)
    with gpu_lib.PigsContext(cfg, VT, WF, n_walkers=1) as ctx:             # beyond half the SHORTEST side: refused
        assert ctx.L.pigs_atm_init(ctx.h, np.nextafter(rc, 2 * rc), 0) == ST["PIGS_ERR_ARG"]
        assert ctx.L.pigs_atm_init(ctx.h, rc, 0) == ST["PIGS_OK"]
        ctx.sync()


@pytest.mark.parametrize("dim", [2, 3])
def test_cutoff_edge(gpu_lib, dim):
    """Box of side 4, rc = 1.5 (rc2 = 2.25), coordinates exactly representable: a pair at r2 == rc2 counts, one ulp beyond
    does not, as the side a2 = (i, j) and as the side c2 = (j, k)."""
    cfg = SystemConfig(dim=dim, Np=3, Nb=1, density=3 / 4.0 ** dim, Lbox=[4.0] * dim)
    assert list(cfg.Lbox[:dim]) == [4.0] * dim
    A, B, Cc = np.zeros(dim), np.zeros(dim), np.zeros(dim)
    B[0] = 1.5                                                          # |A - B|^2 = 2.25 exactly
    Cc[0], Cc[1] = 0.75, 1.0                                            # 0.5625 + 1 = 1.5625 from both
    Bfar = B.copy()
    Bfar[0] = np.nextafter(1.5, 2.0)
    W = 4
    P = np.zeros((W, 3, 3, dim))
    P[0, :] = [A, B, Cc]                                                # the edge pair is (i, j): a2
    P[1, :] = [A, Bfar, Cc]
    P[2, :] = [Cc, A, B]                                                # the edge pair is (j, k): c2
    P[3, :] = [Cc, A, Bfar]
    r2 = pair_r2(P[0, 1], cfg.Lbox)
    assert r2[0, 1] == 2.25 and r2[0, 2] == r2[1, 2] == 1.5625 and pair_r2(P[1, 1], cfg.Lbox)[0, 1] > 2.25
    exp = Window(P, 1, 0, cfg.Lbox).expected(range(W), 1.5)
    assert exp["ntrip"][:, 0].tolist() == [1, 0, 1, 0]
    got = _run_lists(gpu_lib, cfg, P, 1.5, 0, [None])
    assert np.array_equal(got["ntrip"], exp["ntrip"]) and same_bits(got["T"], exp["T"])
    assert got["T"][0, 0] > 0 and got["T"][1, 0] == 0.0 and got["T"][3, 0] == 0.0


# ---- 3. semantics; bits -------------------------------------------------------------------------------------------------
def test_semantics_of_lists_reset_and_reinit(gpu_lib):
    W, Nb, window = 5, 4, 2
    cfg = _cfg(3, 64, Nb)
    VT, WF = gpu_lib.build_tables(cfg)
    P = _paths(cfg, W, np.random.default_rng(5))
    rc = _half(cfg)
    one = _run_lists(gpu_lib, cfg, P, rc, window, [None])
    _assert_same(one, Window(P, Nb, window, cfg.Lbox).expected(range(W), rc), "one call")
    twice = _run_lists(gpu_lib, cfg, P, rc, window, [None, None])         # x + x is exact
    assert same_bits(twice["T"], 2.0 * one["T"]) and twice["samples"].tolist() == [2] * W
    assert np.array_equal(twice["ntrip"], 2 * one["ntrip"])
    dup = _run_lists(gpu_lib, cfg, P, rc, window, [[3, 3]])                # listed twice: counts twice
    assert same_bits(dup["T"][3], 2.0 * one["T"][3]) and dup["samples"].tolist() == [0, 0, 0, 2, 0]
    assert np.array_equal(dup["ntrip"][3], 2 * one["ntrip"][3])
    assert not dup["T"][[0, 1, 2, 4]].any() and not dup["ntrip"][[0, 1, 2, 4]].any()
    with gpu_lib.PigsContext(cfg, VT, WF, n_walkers=W) as ctx:
        ctx.upload_all(P)
        ctx.atm_init(rc, window)
        ctx.atm_accumulate()
        ctx.atm_accumulate([4, 1])                                        # a sub-list leaves the others untouched
        got = ctx.atm_read(reset=[0, 1, 0, 0, 0])
        assert got["samples"].tolist() == [1, 2, 1, 1, 2]
        assert same_bits(got["T"][[0, 2, 3]], one["T"][[0, 2, 3]]) and same_bits(got["T"][[1, 4]], 2.0 * one["T"][[1, 4]])
        assert np.array_equal(got["ntrip"][[1, 4]], 2 * one["ntrip"][[1, 4]])
        after = ctx.atm_read()                                            # the mask zeroed walker 1 only
        assert after["samples"].tolist() == [1, 0, 1, 1, 2] and not after["T"][1].any() and not after["ntrip"][1].any()
        assert same_bits(after["T"][[0, 2, 3, 4]], got["T"][[0, 2, 3, 4]])
        assert np.array_equal(after["ntrip"][[0, 2, 3, 4]], got["ntrip"][[0, 2, 3, 4]])
        ctx.atm_accumulate()                                              # a second init resizes and zeroes, a call in flight
        ctx.atm_init(0.7 * rc, 1)
        z = ctx.atm_read()
        assert z["T"].shape == (W, 3) and not z["T"].any() and not z["ntrip"].any() and not z["samples"].any()
        ctx.atm_accumulate([2])
        _assert_same(ctx.atm_read(), Window(P, Nb, 1, cfg.Lbox).expected([2], 0.7 * rc), "after re-init")


def test_bits_do_not_depend_on_the_launch(gpu_lib):
    W, Nb, window = 5, 3, 1
    cfg = _cfg(3, 65, Nb)
    P = _paths(cfg, W, np.random.default_rng(6))
    rc = _half(cfg)
    ref = _run_lists(gpu_lib, cfg, P, rc, window, [None])
    alone = _run_lists(gpu_lib, cfg, P[4:5], rc, window, [None])          # alone in a context of 1 walker
    assert same_bits(alone["T"][0], ref["T"][4]) and np.array_equal(alone["ntrip"][0], ref["ntrip"][4])
    perm = _run_lists(gpu_lib, cfg, P, rc, window, [[3, 0, 4, 2, 1]])
    assert same_bits(perm["T"], ref["T"]) and np.array_equal(perm["ntrip"], ref["ntrip"])
    split = _run_lists(gpu_lib, cfg, P, rc, window, [[4, 1], [0, 2, 3]])
    assert same_bits(split["T"], ref["T"]) and np.array_equal(split["ntrip"], ref["ntrip"])
    # a list longer than 256 entries (repeats) against the same sums made in short calls
    long_list = [w % W for w in range(300)]
    a = _run_lists(gpu_lib, cfg, P, rc, window, [long_list])
    b = _run_lists(gpu_lib, cfg, P, rc, window, [None] * 60)
    assert a["samples"].tolist() == [60] * W and same_bits(a["T"], b["T"]) and np.array_equal(a["ntrip"], b["ntrip"])
    assert np.array_equal(a["ntrip"], 60 * ref["ntrip"])


def test_more_than_256_walkers_in_one_list(gpu_lib):
    """300 distinct walkers behind one call (two launches) against the same worldlines six at a time."""
    W, Nb, window = 300, 2, 2
    cfg = _cfg(2, 9, Nb)
    P6 = _paths(cfg, 6, np.random.default_rng(11))
    rc = _half(cfg)
    small = _run_lists(gpu_lib, cfg, P6, rc, window, [None])
    big = _run_lists(gpu_lib, cfg, P6[np.arange(W) % 6], rc, window, [None, list(range(W - 1, -1, -1)) + [7, 7, 299]])
    cnt = np.full(W, 2)
    cnt[7] += 2
    cnt[299] += 1
    assert big["samples"].tolist() == cnt.tolist()
    want = np.stack([sum([small["T"][w % 6]] * int(cnt[w] - 1), small["T"][w % 6]) for w in range(W)])
    assert same_bits(big["T"], want) and small["ntrip"].min() > 0
    assert np.array_equal(big["ntrip"], small["ntrip"][np.arange(W) % 6] * cnt[:, None])


# ---- 4. a non-finite element stays local --------------------------------------------------------------------------------
def test_a_coincident_pair_stays_in_its_element(gpu_lib):
    W, Nb, window = 3, 4, 2
    cfg = _cfg(3, 64, Nb)
    P = _paths(cfg, W, np.random.default_rng(8))
    rc = _half(cfg)
    clean = _run_lists(gpu_lib, cfg, P, rc, window, [None])
    assert np.all(np.isfinite(clean["T"]))
    Pb = P.copy()
    a = Nb + 1                                                           # window slice js = 3 of walker 1
    Pb[1, a, 17] = Pb[1, a, 40]
    got = _run_lists(gpu_lib, cfg, Pb, rc, window, [None])
    js = a - (Nb - window)
    assert not np.isfinite(got["T"][1, js])                              # p = 0: the term is not finite
    keep = np.ones((W, 2 * window + 1), bool)
    keep[1, js] = False
    assert np.all(np.isfinite(got["T"][keep])) and same_bits(got["T"][keep], clean["T"][keep])
    assert np.array_equal(got["ntrip"][keep], clean["ntrip"][keep]) and got["samples"].tolist() == [1] * W
    assert got["ntrip"][1, js] == slice_sums(Pb[1, a], cfg.Lbox, rc * rc)[2]


# ---- 5. refusals ------------------------------------------------------------------------------------------------------
def test_status_codes(gpu_lib):
    W, Nb = 2, 3
    ARG, OK, UNS = ST["PIGS_ERR_ARG"], ST["PIGS_OK"], ST["PIGS_ERR_UNSUPPORTED"]
    cfg = _cfg(2, 30, Nb)
    half = _half(cfg)
    VT, WF = gpu_lib.build_tables(cfg)
    l = np.zeros(1 << 10, np.int64).ctypes.data_as(C.POINTER(C.c_int64))
    d = np.zeros(1 << 10).ctypes.data_as(C.POINTER(C.c_double))
    nan, inf = float("nan"), float("inf")
    with gpu_lib.PigsContext(cfg, VT, WF, n_walkers=W) as ctx:
        ctx.upload_all(_paths(cfg, W, np.random.default_rng(2)))
        init = lambda *a: ctx.L.pigs_atm_init(ctx.h, *a)
        with pytest.raises(gpu_lib.PigsError):                            # before init
            ctx.atm_accumulate()
        with pytest.raises(gpu_lib.PigsError):
            ctx.atm_read()
        assert ctx.L.pigs_atm_accumulate(ctx.h, 1, None) == ARG and ctx.L.pigs_atm_read(ctx.h, d, l, l, None) == ARG
        for rc, window in ((0.0, 0), (-1.0, 0), (nan, 0), (inf, 0), (np.nextafter(half, inf), 0), (1.001 * half, 0),
                           (0.5 * half, -1), (0.5 * half, Nb + 1)):
            assert init(rc, window) == ARG, (rc, window)
            with pytest.raises(gpu_lib.PigsError):
                ctx.atm_init(rc, window)
        assert ctx.L.pigs_atm_accumulate(ctx.h, 1, None) == ARG           # init stays undone
        # the limits themselves are accepted
        assert init(1e-300, Nb) == OK and init(half, 0) == OK
        ctx.atm_init(half, Nb)
        for bad in ([2], [-1], [0, 2]):
            with pytest.raises(gpu_lib.PigsError):
                ctx.atm_accumulate(bad)
        assert ctx.L.pigs_atm_accumulate(ctx.h, -1, None) == ARG
        assert ctx.L.pigs_atm_read(ctx.h, None, l, l, None) == ARG and ctx.L.pigs_atm_read(ctx.h, d, None, l, None) == ARG
        assert ctx.L.pigs_atm_read(ctx.h, d, l, None, None) == ARG
        assert ctx.L.pigs_atm_accumulate(ctx.h, W, None) == OK
        assert ctx.atm_read()["samples"].tolist() == [1] * W              # the refused lists added nothing
    # the size limit: slice, leg lists and tail against the budget, the formula of the header; what pigs_g3_init serves
    # (Np <= 975 in 3D) is served
    top = (LDS - TAIL) // (8 * 3 + WAVES * 8 * 4)
    assert top >= 975
    for Np, want in ((975, OK), (top, OK), (top + 1, ARG)):
        big = _cfg(3, Np, 1)
        assert (8 * 3 * Np + WAVES * Np * 8 * 4 + TAIL > LDS) == (want == ARG)
        VT, WF = gpu_lib.build_tables(big)
        with gpu_lib.PigsContext(big, VT, WF, n_walkers=1) as ctx:
            assert ctx.L.pigs_atm_init(ctx.h, _half(big), 0) == want, Np
            if want == ARG:
                assert ctx.L.pigs_atm_accumulate(ctx.h, 1, None) == ARG
            ctx.sync()
    # dim = 1 and trapped contexts: unsupported, a status of its own
    one = SystemConfig(dim=1, Np=6, Nb=2, density=0.2)
    tcfg = SystemConfig(dim=2, Np=6, Nb=2, trap=True, a_ho=[1.0, 1.3], Nmax=2000, Rm=1.2, dt=0.01)
    for c, word in ((one, "2D and 3D"), (tcfg, "periodic")):
        VT, WF = gpu_lib.build_tables(c)
        with gpu_lib.PigsContext(c, VT, WF, n_walkers=1) as ctx:
            assert ctx.L.pigs_atm_init(ctx.h, 0.1, 0) == UNS
            assert ctx.L.pigs_atm_accumulate(ctx.h, 1, None) == ARG            # still before init
            with pytest.raises(gpu_lib.PigsError, match=word):
                ctx.atm_init(0.1)
            ctx.sync()                                                        # the context still works


def test_largest_system_served(gpu_lib):
    """Np at the LDS limit in 3D (a list of Np entries per wave, over 64 KiB of dynamic LDS: the grant path), one slice at
    a first-shell radius against the restatement."""
    top = (LDS - TAIL) // (8 * 3 + WAVES * 8 * 4)
    cfg = _cfg(3, top, 1)
    P = _paths(cfg, 1, np.random.default_rng(top))
    rc = 1.6 * cfg.Lbox[0] / int(np.ceil(top ** (1.0 / 3) - 1e-9))
    exp = Window(P, 1, 0, cfg.Lbox).expected([0], rc)
    got = _run_lists(gpu_lib, cfg, P, rc, 0, [None])
    _assert_same(got, exp, f"Np {top}")
    assert exp["ntrip"].min() > top


# ---- 6. the front end -------------------------------------------------------------------------------------------------
PRINT = 1.0000001e-9            # the files carry 10 significant digits


@pytest.fixture(scope="module")
def exe(gpu_lib):
    import subprocess
    host = os.path.join(ROOT, "pathintegralgroundstate_amd", "host")
    subprocess.check_call(["make", "-s", "-C", host])
    return os.path.join(host, "pigs_vpi")


def test_front_end_two_blocks_three_steps(gpu_lib, oracle, exe, tmp_path):
    """he4_cworm0 (2D, periodic, CWorm = 0: every step is a diagonal one), 2 blocks x 3 steps, two walkers, three_body = T:
    the old files byte for byte, the shapes of v3_vpi.out and v3tau_vpi.out, tau = (a - Nb) dt, the block file's window
    mean against the slice file's column, P3 against pressure_atm, and every number against a replay of the run's chains
    through PigsContext.atm_* and normalize_atm."""
    from test_gpu_front_end_blocks import _input, _run as run_vpi, replay
    W, Nblock, Nstep, window, nu = 2, 2, 3, 2, 0.625
    txt, cfg = _input("he4_cworm0", Nblock, Nstep)
    Nb, ns = cfg.Nb, 2 * window + 1
    key = f", three_body = T, atm_nu = {nu!r}, atm_window = {window}"
    plain, on = str(tmp_path / "plain"), str(tmp_path / "on")
    run_vpi(exe, txt + f"&gpu\n n_walkers = {W}\n/\n", plain)
    out = run_vpi(exe, txt + f"&gpu\n n_walkers = {W}{key}\n/\n", on)
    assert "Three-body V3" in out and "bare geometric sum" not in out
    old = sorted(os.listdir(plain))
    new = sorted(set(os.listdir(on)) - set(old))
    assert sorted(f for f in new if ".w" not in f) == ["v3_vpi.out", "v3tau_vpi.out"] and len(new) == 2 + 2 * W, new
    for f in old:
        if f not in ("stdout.txt", "vpi.in"):
            assert open(os.path.join(plain, f), "rb").read() == open(os.path.join(on, f), "rb").read(), f
    rep = replay(gpu_lib, oracle, cfg, W, Nblock, Nstep)
    final = np.fromfile(os.path.join(on, "worldlines_final.bin")).reshape(rep["final"].shape)
    assert np.array_equal(final, rep["final"]) and rep["diag"].all()
    VT, WF = gpu_lib.build_tables(cfg)
    V3 = np.zeros((W, Nblock, ns))
    NT = np.zeros((W, Nblock, ns))
    AB = np.zeros((W, Nblock, ns))                                       # Sum|t| per particle and sample: the scale of V3's error
    with gpu_lib.PigsContext(cfg, VT, WF, n_walkers=W) as ctx:
        ctx.atm_init(cfg.rcut, window)                                    # atm_rc left out: half the side, the run's rcut
        for b in range(Nblock):
            snaps = rep["snaps"][b * Nstep:(b + 1) * Nstep]
            for P in snaps:
                ctx.upload_all(P)
                ctx.atm_accumulate()
                AB[:, b] += abs(nu) * Window(P, Nb, window, cfg.Lbox).expected(range(W), cfg.rcut)["abs"] / (Nstep * cfg.Np)
            n = normalize_atm(ctx.atm_read(reset=True), cfg.Np, nu)
            V3[:, b], NT[:, b] = n["v3"], n["ntrip"]
    assert NT.min() >= 1 and not np.array_equal(V3[0, 0], V3[0, 1])
    a = np.arange(Nb - window, Nb + window + 1)
    names = sorted(f for f in new if re.fullmatch(r"v3_vpi\.w\d+\.out", f))
    assert len(names) == W
    for w, fb, ft, v3, nt, ab in [(w, f, f.replace("v3_", "v3tau_"), V3[w], NT[w], AB[w]) for w, f in enumerate(names)] + \
                                 [(None, "v3_vpi.out", "v3tau_vpi.out", V3.mean(axis=0), NT.mean(axis=0), AB.mean(axis=0))]:
        blk = np.loadtxt(os.path.join(on, fb), ndmin=2)
        tau = np.loadtxt(os.path.join(on, ft), ndmin=2)
        assert blk.shape == (Nblock, 3) and tau.shape == (ns, 5), (fb, blk.shape, tau.shape)
        assert blk[:, 0].tolist() == [1.0, 2.0] and np.array_equal(tau[:, 0], a)
        assert np.allclose(tau[:, 1], (a - Nb) * cfg.dt, rtol=PRINT, atol=0)              # tau = (a - Nb) dt
        scale = np.abs(v3).mean(axis=1)                                                     # per block
        # the window mean of every block, and the slice column as the mean over the blocks
        assert np.all(np.abs(blk[:, 1] - v3.mean(axis=1)) <= PRINT * scale + 1e-12 * ab.mean(axis=1)), fb
        assert np.all(np.abs(tau[:, 2] - v3.mean(axis=0)) <= PRINT * np.abs(v3).mean(axis=0) + 1e-12 * ab.mean(axis=0)), ft
        assert np.allclose(tau[:, 4], nt.mean(axis=0), rtol=PRINT, atol=0), ft
        err = np.sqrt(np.maximum((v3 * v3).mean(axis=0) - v3.mean(axis=0) ** 2, 0.0) / Nblock)
        m = np.abs(v3).mean(axis=0)
        assert np.all(np.abs(tau[:, 3] - err) <= np.sqrt(4.0 * m * (PRINT * m + 1e-12 * ab.mean(axis=0))) + PRINT * err), ft
        # the two files against each other, to the printed digits: mean over the blocks of the window mean = mean over
        # the window of the slice column
        assert abs(blk[:, 1].mean() - tau[:, 2].mean()) <= PRINT * (np.abs(blk[:, 1]).mean() + np.abs(tau[:, 2]).mean()), (fb, ft)
        # P3 is pressure_atm of the V3/N column
        assert np.allclose(blk[:, 2], pressure_atm(blk[:, 1], cfg.density, cfg.dim), rtol=2 * PRINT, atol=0), fb
    # atm_nu left out: the banner says so and the files hold the bare geometric sum, the run above divided by nu
    bare = str(tmp_path / "bare")
    out = run_vpi(exe, txt + f"&gpu\n n_walkers = {W}, three_body = T, atm_window = {window}\n/\n", bare)
    assert "bare geometric sum" in out
    t1, tn = np.loadtxt(os.path.join(bare, "v3tau_vpi.out"), ndmin=2), np.loadtxt(os.path.join(on, "v3tau_vpi.out"), ndmin=2)
    assert np.allclose(t1[:, 2] * nu, tn[:, 2], rtol=3 * PRINT, atol=0) and np.array_equal(t1[:, 4], tn[:, 4])


@pytest.mark.parametrize("extra,word", [(", atm_rc = 1.d3", "atm_rc"), (", atm_window = 1000", "atm_window")])
def test_front_end_refuses_bad_keys_before_any_gpu_work(gpu_lib, exe, tmp_path, extra, word):
    import subprocess
    from test_gpu_front_end_blocks import _input
    txt, _ = _input("he4_cworm0", 1, 1)
    wd = str(tmp_path)
    with open(os.path.join(wd, "vpi.in"), "w") as f:
        f.write(txt + f"&gpu\n three_body = T{extra}\n/\n")
    with open(os.path.join(wd, "vpi.in")) as fin:
        r = subprocess.run([exe], stdin=fin, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, cwd=wd, timeout=120)
    out = r.stdout.decode(errors="replace")
    assert r.returncode == 2 and "three_body" in out and word in out, out[-2000:]
    assert not os.path.exists(os.path.join(wd, "e_vpi.out"))
